"""The loss math of csrc/device_math.h at its call sites, on prescribed inputs, against the extended-precision reference
of tests/lossmath_ref.py (certified on the CPU by test_lossmath_host.py).  Every comparison is per element,
|got - ref| <= bar eps scale(ref_i, m_i) with eps = 2^-52 and scale = max(1, |x*|, |m|) (hinge: and sigma / rho); the bars
are lossmath_ref.BAR (element prox: 16 BCE, bit-equal hinge, 4 squared hinge) and BAR_PAV (32: a pooled block).

  a  rbl_k_prox                      prox_bce / prox_hinge / prox_sqhinge, cold            (elementwise.hip: k_prox)
  b  rbl_k_sweep_erm                 prox_bce_warm from a prescribed z_old, both kernels    (sweep_erm.hip:202, :414)
  c  phase_m / phase_z / phase_q     k_erm_zc, RS = false and RS = true, f64 and csr        (elementwise.hip:35)
  d  rbl_k_pav                       prox_est at level 0, block_value of pooled blocks      (pav.hip:607, :150)
  e  rbl_k_pav_ehrm, three modes     softplus_near, the threshold shortcut, k_ehrm_fvals    (pav.hip:585-603, :945)
  f  phase_dual / phase_finish       k_dual, k_sum_partials, k_pack_stats, launch_loss_sum  (elementwise.hip:203, api_iter.hip:595)
  g  rbl_k_prox                      monotone in m

Not reachable with prescribed inputs, no back door added: a NaN warm start in the single-sweep kernels (z_old also
enters lambda' = lambda + rho (z_old - v), so m would be NaN as well), and the two f-values of the EHRM test (no entry
returns them: the branch they decide is compared instead).  Each test prints its largest error / bar (pytest -s)."""
import numpy as np
import pytest

import lossmath_ref as R
import sweep_fixtures as F

pytestmark = pytest.mark.gpu

LD = R.LD
DOT = F.DOT                       # x (absolute sum + 1): an fp64 dot product or column sum (test_gemv_gemvt)
RISK_BAR = 1e-12                  # tests/risk_fixtures.py: BAR, relative to max(1, |ref|)


@pytest.fixture(scope="module")
def rbl():
    import admm_for_rank_based_loss_amd as pkg
    if pkg._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return pkg


@pytest.fixture(scope="module")
def L(rbl):
    return rbl._lib


@pytest.fixture(scope="module")
def tab():
    sigma, rho, m = R.tables()
    return dict(sigma=sigma, rho=rho, m=m, x={loss: R.prox(loss, sigma, rho, m) for loss in R.LOSSES})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hinge_numpy(sigma, rho, m):
    """one IEEE division, one subtraction, two comparisons: what the device must return bit for bit"""
    a = m - sigma / rho
    return np.where(a >= -1.0, a, np.where(m <= -1.0, m, -1.0))


def check(site, loss, got, ref, sc, ctx="", bar=None, sigma=None, rho=None, m=None):
    """per element within bar eps scale; the hinge (bar 0) against NumPy's bits as well.  -> largest error / bar"""
    bar = R.BAR[loss] if bar is None else bar
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), (site, loss, ctx, "not finite", np.flatnonzero(~np.isfinite(got))[:5])
    e = R.err_units(got, ref, sc)
    k = int(np.argmax(e)) if e.size else 0
    worst = float(e[k]) if e.size else 0.0
    if bar == 0.0:
        want = hinge_numpy(sigma, rho, m)
        same = bits(got) == bits(want)
        print(f"lossmath-ratio {site} {loss} {ctx}: {int(np.count_nonzero(~same))} of {got.size} differ from NumPy's bits; "
              f"{worst:.3f} eps scale from the exact value")
        assert np.all(same), (site, loss, ctx, np.flatnonzero(~same)[:5])
        assert worst <= R.BAR_ORACLE[loss], (site, loss, ctx, worst)
        return 0.0
    print(f"lossmath-ratio {site} {loss} {ctx}: worst {worst:.3f} eps scale = {worst / bar:.3f} of the bar {bar:g}"
          + (f" (element {k}, ref {float(ref[k]):.17g})" if e.size else ""))
    assert worst <= bar, (site, loss, ctx, k, worst, float(got[k]), float(ref[k]))
    return worst / bar


# ------------------------------------------------------------------------------------------------ a. rbl_k_prox, cold
@pytest.mark.parametrize("loss", R.LOSSES)
def test_a_prox_cold_start(L, tab, loss):
    sigma, rho, m, x = tab["sigma"], tab["rho"], tab["m"], tab["x"][loss]
    got = np.full(m.size, np.nan)
    for r in np.unique(rho):
        k = np.flatnonzero(rho == r)
        got[k] = L.k_prox(loss, sigma[k], r, m[k])
        if k.size >= 65:                      # a single element, a wave less one, a wave, a wave and one
            for n in (1, 63, 64, 65):
                assert np.array_equal(bits(L.k_prox(loss, sigma[k[:n]], r, m[k[:n]])), bits(got[k[:n]])), (loss, r, n)
    check("k_prox", loss, got, x, R.scale_of(loss, x, sigma, rho, m), f"{m.size} elements", sigma=sigma, rho=rho, m=m)
    zero = sigma == 0
    assert zero.sum() >= 50 and np.array_equal(bits(got[zero]), bits(m[zero])), (loss, "sigma = 0 must return m itself")


# ------------------------------------------------------------------------------------------------ g. monotone in m
@pytest.mark.parametrize("loss", R.LOSSES)
def test_g_prox_is_monotone_in_m(L, tab, loss):
    """constant sigma, sorted m (the tables' values, and 200 consecutive doubles around each kink): the hinge and the
    squared hinge never decrease (device_math.h claims it of the computed values); BCE decreases by less than its bar"""
    worst = 0.0
    for sigma, rho in ((1e-3, 1.0), (0.5, 2.0 ** -22), (3.0, 1.0), (1e-2, 2.0 ** 10), (0.3, 2.0 ** -3)):
        a = sigma / rho
        runs = [tab["m"]]
        for c in (-1.0, -1.0 + a, -1.0 + 2 * a, 0.0, a):
            v = [c]
            for _ in range(100):
                v.append(np.nextafter(v[-1], np.inf))
            for _ in range(100):
                v.insert(0, np.nextafter(v[0], -np.inf))
            runs.append(np.array(v))
        m = np.unique(np.concatenate(runs))
        u = L.k_prox(loss, np.full(m.size, sigma), rho, m)
        drop = np.maximum(u[:-1] - u[1:], 0.0)
        if loss == R.BCE:
            x = R.prox_bce(sigma, rho, m)
            units = np.asarray(LD(1) * drop / (LD(R.EPS) * R.scale(x, m)[1:]), dtype=np.float64)
            worst = max(worst, float(units.max()))
            assert units.max() <= R.BAR[loss], (sigma, rho, int(np.argmax(units)))
        else:
            assert not drop.any(), (loss, sigma, rho, np.flatnonzero(drop)[:5])
    print(f"lossmath-ratio monotone {loss}: largest decrease {worst:.3f} eps scale = {worst / 16.0:.3f} of the bar")


# ------------------------------------------------------------------------------------------------ b. prox_bce_warm
SWEEP_CASES = [("f64", F._FUSED_WAVE[0]), ("f64", F._FUSED_WIDE[0]), ("f32", F._FUSED_WIDE[0])]
Z_OLD = ("root", "root(1+1e-6)", "root(1-1e-6)", "root+1e-3", "root-1e-3", "m", "m-sigma/rho", "far below", "far above")


def _sweep_inputs(sigma0, rho_next, seed):
    """rows (m target, z_old): every m of the grid and 31 draws in +-50, each with every kind of warm start"""
    rng = np.random.default_rng(seed)
    mt = np.repeat(np.concatenate([R.GRID_M, rng.uniform(-50, 50, 31)]), len(Z_OLD))
    kind = np.tile(np.arange(len(Z_OLD)), mt.size // len(Z_OLD))
    root = np.asarray(R.prox_bce(sigma0, rho_next, mt), dtype=np.float64)
    a = sigma0 / rho_next
    far = 50.0 + a + np.abs(mt)
    z = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7],
                  [root, root * (1 + 1e-6), root * (1 - 1e-6), root + 1e-3, root - 1e-3, mt, mt - a, mt - a - far], mt + far)
    return mt, z, kind


@pytest.mark.parametrize("case", SWEEP_CASES, ids=F.case_id)
def test_b_warm_prox_in_the_single_sweep_kernels(L, case):
    """w = 0 makes v = 0 exactly; rho and rho_next are powers of two, so lambda' = lambda + rho z_old has one rounding and
    m = -lambda' / rho_next none: the reference is built from the lambda' that comes back.  One call per decade pair of
    sigma0 / rho_next; z' within the BCE bar whatever the warm start, sum z'^2 within the bound of test_gpu_sweep.py."""
    st, inst = case
    d = F.widths(st, inst)[0]
    rng = np.random.default_rng(d)
    worst, per_kind = 0.0, np.zeros(len(Z_OLD))
    for j, ratio in enumerate(R.GRID_RATIO):
        rho_next = float(R.GRID_RHO[j % len(R.GRID_RHO)])
        rho, sigma0 = rho_next / 2.0, float(ratio * rho_next)
        mt, z_old, kind = _sweep_inputs(sigma0, rho_next, j)
        n = mt.size
        D = F.storage_round(rng.standard_normal((n, d)), st)
        lam = -rho_next * mt - rho * z_old
        out = L.k_sweep_erm(D, np.zeros(d), z_old, lam, sigma0, rho, rho_next, R.BCE, st, 1)
        assert out["instance"] == F.reported("fused", inst, 1), (case, out["instance"])
        assert not out["v"].any() and np.array_equal(out["lam"], lam + rho * z_old), (case, ratio)
        m = -out["lam"] / rho_next
        x = R.prox_bce(sigma0, rho_next, m)
        sc = R.scale(x, m)
        e = R.err_units(out["z"], x, sc)
        assert np.all(np.isfinite(out["z"])), (case, ratio, np.flatnonzero(~np.isfinite(out["z"]))[:5])
        for k in range(len(Z_OLD)):
            per_kind[k] = max(per_kind[k], float(e[kind == k].max()))
        i = int(np.argmax(e))
        worst = max(worst, float(e[i]))
        assert e[i] <= R.BAR[R.BCE], (case, ratio, Z_OLD[kind[i]], float(m[i]), float(out["z"][i]), float(x[i]), float(e[i]))
        e_z = np.asarray(R.BAR[R.BCE] * LD(R.EPS) * sc, dtype=np.float64)
        zz = float(np.sum(x * x))
        e_zz = float(np.sum(2.0 * np.abs(out["z"]) * e_z + e_z ** 2)) + DOT * (zz + 1.0)
        assert abs(out["zz"] - zz) <= e_zz, (case, ratio, out["zz"], zz, e_zz)
    print(f"lossmath-ratio sweep_erm {F.case_id(case)} d={d} BCE: worst {worst:.3f} eps scale = {worst / 16.0:.3f} of the bar; "
          + " ".join(f"[{nm}] {v:.2f}" for nm, v in zip(Z_OLD, per_kind)))
    # the closed forms in the same kernels, once each
    for loss in (R.HINGE, R.SQ):
        rho_next, rho, sigma0 = 0.25, 0.5, 0.75
        mt, z_old, _ = _sweep_inputs(sigma0, rho_next, 99)
        mt = np.concatenate([mt, [-1.0, -1.0 + 3.0, np.nextafter(2.0, 3.0), np.nextafter(2.0, 1.0), np.nextafter(-1.0, 0.0)]])
        z_old = np.concatenate([z_old, np.zeros(5)])
        D = F.storage_round(rng.standard_normal((mt.size, d)), st)
        out = L.k_sweep_erm(D, np.zeros(d), z_old, -rho_next * mt - rho * z_old, sigma0, rho, rho_next, loss, st, 1)
        m = -out["lam"] / rho_next
        x = R.prox(loss, sigma0, rho_next, m)
        check("sweep_erm " + F.case_id(case), loss, out["z"], x, R.scale_of(loss, x, sigma0, rho_next, m), f"d={d}",
              sigma=np.full(m.size, sigma0), rho=rho_next, m=m)


# ------------------------------------------------------------------------------------------------ handles for c and f
def _read(rbl, s, which, count):
    import torch
    from admm_for_rank_based_loss_amd.dist import _DevArray
    ptr, cnt = s.buffer(which)
    torch.cuda.synchronize()
    assert cnt >= count, (which, cnt, count)
    return torch.as_tensor(_DevArray(ptr, cnt), device=torch.device("cuda", 0)).cpu().numpy()[:count].copy()


REG = 2.0 ** -7


def _handles(rbl, monkeypatch, X, y, loss, storage, y_own=None):
    """an erm handle on (X, y) that runs the plain kernels (RBL_NO_FUSE is read at create; storage="csr" has no fused
    pass at all), and, with y_own, a borrower of its D with those labels (RS = true)"""
    monkeypatch.setenv("RBL_NO_FUSE", "1")
    n, d = X.shape
    own = rbl.Solver(n, d, "erm", loss, reg=REG, wstep=2, tol=0.0, storage=storage)
    if storage == "csr":
        import torch
        own.set_data(torch.from_numpy(X).to_sparse_csr(), y)
    else:
        own.set_data(X, y)
    if y_own is None:
        return own, None
    own.gram()                                        # a borrower takes the owner's Gram matrix with its D
    bor = rbl.Solver(n, d, "erm", loss, reg=REG, wstep=2, tol=0.0, storage=storage, share=own)
    bor.set_labels(y_own)
    return own, bor


def _small_problem(n, seed):
    rng = np.random.default_rng([seed, n])
    X = rng.integers(-3, 4, size=(n, 3)).astype(np.float64)
    X[:, 0] += (X[:, 0] == 0)                         # no empty row in the sparse storage
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    y2 = y.copy()
    y2[rng.permutation(n)[: n // 2]] *= -1.0          # half of the labels flipped
    return X, y, y2


# ------------------------------------------------------------------------------------------------ c. k_erm_zc
ZC_RHO = (2.0 ** -20, 2.0 ** -4, 1.0, 2.0 ** 10)      # sigma0 / rho = 1 / (n rho): 1e-7 .. 4e3; lambda stays normal at 1e-300


@pytest.mark.parametrize("storage", ["f64", "csr"])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_c_erm_zstep_through_the_phases(rbl, monkeypatch, loss, storage):
    """set_state(w = 0, lambda = -rho m0) -> phase_m, phase_z: m has m0's bits, z is the element prox at sigma0 = 1 / n;
    c = z + lambda / rho shows through phase_q: q = D^T c for a D of small integers, under the bound of the plain passes.
    The borrower (half of the labels flipped) gets the same m0 in its own sign convention: the same z, and the q of
    r (z + lambda / rho) on the owner's D."""
    from admm_for_rank_based_loss_amd import _lib
    worst = {False: 0.0, True: 0.0}
    for n in (255, 256, 257, 4099):
        X, y, y2 = _small_problem(n, 3)
        D = -y[:, None] * X
        own, bor = _handles(rbl, monkeypatch, X, y, loss, storage, y2)
        m0 = R.edge_m(n)
        for rho in ZC_RHO:
            lam = -rho * m0
            x = R.prox(loss, 1.0 / n, rho, m0)
            sc = R.scale_of(loss, x, 1.0 / n, rho, m0)
            for s, r in ((own, np.ones(n)), (bor, y2 * y)):
                rs = s is bor
                ctx = f"{storage} n={n} rho=2^{int(np.log2(rho))} RS={rs}"
                s.set_state(w=np.zeros(3), lam=lam, rho=rho)
                s.phase_m()
                s.phase_z()
                m = _read(rbl, s, _lib.BUF_M, n)
                nz = m0 != 0                  # (the zero of m0 comes back as -0.0 where the borrower's sign is -1)
                assert np.array_equal(m, m0) and np.array_equal(bits(m[nz]), bits(m0[nz])), (ctx, "m was not injected exactly")
                z = s.get_state(want_lam=False)["z"].copy()
                worst[rs] = max(worst[rs], check("k_erm_zc", loss, z, x, sc, ctx, sigma=np.full(n, 1.0 / n), rho=rho, m=m0))
                s.phase_q()
                q = _read(rbl, s, _lib.BUF_Q, 3)
                c = r * (z + lam / rho)
                q_ref = np.asarray(D.T.astype(LD) @ c.astype(LD), dtype=np.float64)
                e_q = DOT * (np.abs(D).T @ np.abs(c) + 1.0)
                assert np.all(np.abs(q - q_ref) <= e_q), (ctx, q, q_ref, e_q)
                s.phase_w()
                s.phase_dual(False)
                s.phase_finish()
        bor.close()
        own.close()
    print(f"lossmath-ratio k_erm_zc {loss} {storage}: RS=false {worst[False]:.3f} RS=true {worst[True]:.3f} of the bar")


# ------------------------------------------------------------------------------------------------ d. PAV
def _pav_check(L, loss, kind, n=None):
    sigma, m, seg = R.pav_design(kind, n)
    worst = 0.0
    for rho in R.PAV_RHO:
        pos, x, sc = R.pav_reference(loss, sigma, rho, m, seg)
        u, merges = L.k_pav(loss, sigma, rho, m)
        ctx = f"{kind} n={m.size} rho=2^{int(np.log2(rho))}"
        if loss == R.HINGE:
            assert np.all(np.isfinite(u))
            e = R.err_units(u, pos, sc)
            print(f"lossmath-ratio k_pav {loss} {ctx}: worst {e.max():.3f} eps scale = {e.max() / R.BAR_PAV:.3f} of the bar")
            assert e.max() <= R.BAR_PAV, (ctx, float(e.max()))
            worst = max(worst, float(e.max()) / R.BAR_PAV)
        else:
            worst = max(worst, check("k_pav", loss, u, pos, sc, ctx, bar=R.BAR_PAV))
        assert np.all(np.diff(u) >= 0), ctx
        strict = R.pav_strict_segments(loss, sigma, rho, m, seg)
        sure = int(np.sum((seg - 1)[strict]))
        assert sure <= merges <= m.size - seg.size, (ctx, merges, sure, m.size - seg.size)
        ends = np.cumsum(seg)
        for a, b, ok in zip(ends - seg, ends, strict):
            if ok:
                assert np.all(u[a:b] == u[a]), (ctx, "a segment that pools strictly is one block", a, b)
    return worst


@pytest.mark.parametrize("loss", [R.BCE, R.SQ])
def test_d_pav_level0_and_pooled_blocks(L, loss):
    """dyadic inputs (exact prefix sums): no pooling -> the element prox from the series estimate; one block of n; the
    segments of lossmath_ref.PAV_SEG_LEN, one of them across position 2048.  n_merges: a segment of k positions that
    pools strictly costs k - 1 merges, so n - segments when all do."""
    w = [_pav_check(L, loss, "separate"), _pav_check(L, loss, "segments")]
    w += [_pav_check(L, loss, "one_block", n) for n in R.PAV_ONE_BLOCK_N]
    print(f"lossmath-ratio k_pav {loss}: worst {max(w):.3f} of the bar {R.BAR_PAV:g}")


def test_d_pav_one_block_hinge(L):
    w = [_pav_check(L, R.HINGE, "one_block", n) for n in R.PAV_ONE_BLOCK_N]
    print(f"lossmath-ratio k_pav hinge: worst {max(w):.3f} of the bar {R.BAR_PAV:g}")


# ------------------------------------------------------------------------------------------------ e. EHRM
MODES = [None, "0", "-1"]


def _ehrm_all_modes(L, monkeypatch, B, rho, m):
    sa, sb = R.ehrm_weights()
    out = []
    for mode in MODES:
        if mode is None:
            monkeypatch.delenv("RBL_EHRM_SPEC", raising=False)
        else:
            monkeypatch.setenv("RBL_EHRM_SPEC", mode)
        out.append(L.k_pav_ehrm(sa, sb, B, rho, m))
    monkeypatch.delenv("RBL_EHRM_SPEC", raising=False)
    return out


@pytest.mark.parametrize("rho", R.EHRM_RHO, ids=["softplus", "expansion"])
@pytest.mark.parametrize("B", R.EHRM_B)
def test_e_ehrm_branch_in_every_mode(L, monkeypatch, B, rho):
    """the singleton-stage test (f1 <= f2) from longdouble roots and sums; the designs keep the two apart by far more than
    a float64 sum of 2049 terms can be wrong (test_lossmath_host.py).  Speculating b (default), speculating a and the
    separate test kernel must all choose the reference's branch, and return the same bits when they agree."""
    m = R.ehrm_design(B, rho)
    ref = R.ehrm_reference(B, rho, m)
    res = _ehrm_all_modes(L, monkeypatch, B, rho, m)
    print(f"lossmath-ratio ehrm B={B} rho=2^{int(np.log2(rho))}: reference branch {ref['branch']} "
          f"(f1 - f2 = {float(ref['f1'] - ref['f2']):.6e}), device {[br for _, br in res]}")
    worst_drop = 0.0
    for (z, br), mode in zip(res, MODES):
        assert br == ref["branch"], (B, rho, mode, br, float(ref["f1"]), float(ref["f2"]))
        assert np.all(np.isfinite(z)), (B, rho, mode)
        # neighbouring blocks whose exact values differ by less than their rounding may come out in the wrong order (the
        # thresholds' positions pool into blocks that all sit on B to 1e-13): by less than the pooled block's bar
        drop = np.asarray(np.maximum(z[:-1] - z[1:], 0.0) / (LD(R.EPS) * R.scale(z, m)[1:]), dtype=np.float64)
        worst_drop = max(worst_drop, float(drop.max()))
        assert drop.max() <= R.BAR_PAV, (B, rho, mode, "z decreases", int(np.argmax(drop)), float(drop.max()))
        assert np.all(z <= B) if br == 0 else np.all(z >= B), (B, rho, mode)
    for (z, br), mode in zip(res[1:], MODES[1:]):
        assert np.array_equal(bits(z), bits(res[0][0])), (B, rho, mode, "the modes differ in bits")
    print(f"lossmath-ratio ehrm B={B} rho=2^{int(np.log2(rho))}: largest decrease of z {worst_drop:.3f} eps scale = "
          f"{worst_drop / R.BAR_PAV:.3f} of the bar {R.BAR_PAV:g}")


def test_e_ehrm_close_call(L, monkeypatch):
    """f1 below f2 by 5e-9 of their sum, f1 computed through the expansion of softplus at |prox - m| up to 0.1 (the design
    and its tuning: lossmath_ref.EHRM_CLOSE): every mode must still choose branch a, and return the same bits"""
    B, rho, m = R.ehrm_close_call()
    ref = R.ehrm_reference(B, rho, m)
    res = _ehrm_all_modes(L, monkeypatch, B, rho, m)
    print(f"lossmath-ratio ehrm close call: reference branch {ref['branch']} "
          f"((f1 - f2) / (f1 + f2) = {float((ref['f1'] - ref['f2']) / (ref['f1'] + ref['f2'])):.3e}), device {[br for _, br in res]}")
    for (z, br), mode in zip(res, MODES):
        assert br == ref["branch"] == 0, (mode, br)
        assert np.array_equal(bits(z), bits(res[0][0])), (mode, "the modes differ in bits")


@pytest.mark.parametrize("B", R.EHRM_B)
def test_e_ehrm_without_pooling_is_the_clipped_element_prox(L, monkeypatch, B):
    rho = R.EHRM_MONO_RHO
    m = R.ehrm_monotone(B)
    ref = R.ehrm_reference(B, rho, m)
    want = ref["o1"] if ref["branch"] == 0 else ref["o2"]
    res = _ehrm_all_modes(L, monkeypatch, B, rho, m)
    for (z, br), mode in zip(res, MODES):
        assert br == ref["branch"], (B, mode)
        check("k_pav_ehrm", R.BCE, z, want, R.scale(want, m), f"B={B} mode={mode}")
        assert np.array_equal(bits(z), bits(res[0][0])), (B, mode)
    for forced, o in ((0, ref["o1"]), (1, ref["o2"])):
        sa, sb = R.ehrm_weights()
        z, br = L.k_pav_ehrm(sa, sb, B, rho, m, branch=forced)
        assert br == forced
        check("k_pav_ehrm", R.BCE, z, o, R.scale(o, m), f"B={B} forced branch {forced}")


# ------------------------------------------------------------------------------------------------ f. k_dual
DUAL_N = (1, 255, 257, 262143, 262144, 262145, 524289)     # 1024 x 256 threads: a thread loops from 262 145 on
DUAL_RHO = 2.0 ** -3


def _dual_case(rbl, monkeypatch, loss, storage, n, relabel):
    rng = np.random.default_rng([n, len(loss)])
    v = R.edge_m(n, seed=n)
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    X = rng.integers(-3, 4, size=(n, 3)).astype(np.float64)
    X[:, 0] = -y * v                                         # column 0 of D = -y X is v, bit for bit
    y2 = y.copy()
    y2[rng.permutation(n)[: n // 2]] *= -1.0
    own, bor = _handles(rbl, monkeypatch, X, y, loss, storage, y2 if relabel else None)
    s, r = (bor, y2 * y) if relabel else (own, np.ones(n))
    v_own = r * v                                            # what the handle's own losses and residuals see
    z = v_own + rng.standard_normal(n)
    lam = rng.standard_normal(n)
    s.set_state(w=np.zeros(3), lam=lam, rho=DUAL_RHO)
    s.phase_z_external(z)
    s.phase_q()
    s.phase_w_external(np.array([1.0, 0.0, 0.0]))
    s.phase_dual(True)
    st = s.phase_finish()
    ctx = (loss, storage, n, relabel)
    assert st.fused == 0 and st.fused_v == 0, (ctx, "the plain pair gemv + k_dual did not run")
    got = s.get_state()
    lam_ref = lam + DUAL_RHO * (z - v_own)
    assert np.array_equal(bits(got["lam"]), bits(lam_ref)), (ctx, np.flatnonzero(got["lam"] != lam_ref)[:5])
    res = LD(1) * z - LD(1) * v_own
    p2 = float(np.sum(res * res))
    e_p2 = DOT * (p2 + 1.0) + 8 * R.EPS * p2
    assert abs(st.primal ** 2 - p2) <= e_p2 + 4 * R.EPS * p2, (ctx, st.primal ** 2, p2)
    risk = np.sum(R.sample_loss(loss, v_own)) / n
    obj = float(risk + LD(0.5 * REG))
    err = abs(st.objective - obj) / max(1.0, abs(obj))
    assert np.isfinite(st.objective) and err <= RISK_BAR, (ctx, st.objective, obj, err)
    if bor is not None:
        bor.close()
    own.close()
    return abs(st.primal ** 2 - p2) / e_p2, err / RISK_BAR


@pytest.mark.parametrize("storage", ["f64", "csr"])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_f_dual_update_and_statistics(rbl, monkeypatch, loss, storage):
    """set_state(lambda, rho), an external z, phase_q, an external w = e_1 (so v is column 0 of D, which carries the edge
    table), phase_dual with the objective, phase_finish: lambda' = lambda + rho (z - v) bit for bit (rho a power of
    two; the library is built without fma contraction), the primal residual and the objective's loss term against
    longdouble sums."""
    w = [_dual_case(rbl, monkeypatch, loss, storage, n, False) for n in DUAL_N]
    print(f"lossmath-ratio k_dual {loss} {storage}: primal^2 {max(a for a, _ in w):.3f} of its bound, "
          f"objective {max(b for _, b in w):.3f} of the bar {RISK_BAR:g}")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_f_dual_of_a_relabelled_member_with_the_objective(rbl, monkeypatch, loss):
    """RS = true with objective logging: k_dual sums the losses at v as the pass left it, launch_loss_sum replaces them
    by the losses at r v (api_iter.hip: rbl_phase_dual)"""
    a, b = _dual_case(rbl, monkeypatch, loss, "f64", 262145, True)
    print(f"lossmath-ratio k_dual RS=true {loss}: primal^2 {a:.3f} of its bound, objective {b:.3f} of the bar {RISK_BAR:g}")
