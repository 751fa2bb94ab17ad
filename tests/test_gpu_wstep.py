"""Every route and kernel instance of run_wstep (csrc/wstep.hip, csrc/lasso_fs.hip) on prescribed G and q, through
rbl_k_wstep_seq: the entry runs run_wstep as the solver does, K steps on one workspace, and reports which form and which
kernel instance ran.  Fixtures, planted minimisers and bounds: tests/wstep_fixtures.py (checked on the CPU by
tests/test_wstep_host.py).  Three layers:
  exact     integer G, w0, q with a first residual of exactly zero: 0 iterations, w = w0 and G w bit for bit
  planted   a chosen minimiser w*, q formed from it in longdouble: true residual, error in w and G w within derived bounds
  sequence  12 drifting right-hand sides on one workspace: tags, buffer parity, batch sizes, back-off, the wrap of launch_seq
A test that expects the persistent route FAILS when a batched launch ran instead (a solver handle another module left
alive makes wp_plan choose it: the report's live_handles says so)."""
import gc

import numpy as np
import pytest

import wstep_fixtures as F

pytestmark = pytest.mark.gpu

TOL = 1e-13
RHO, REG, T = 1.0, 0.5, 0.5
GEMV = 1e-13                      # |y - G w| <= GEMV (|G| |w| + 1): the constant of test_gemv_gemvt


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    gc.collect()                  # solver handles of earlier modules that only wait for the collector
    return rbl._lib


@pytest.fixture(scope="module")
def ratios():
    """largest error / bound per route, printed when the module ends (pytest -s)"""
    r = {}
    yield r
    for k in sorted(r):
        print(f"w-step error/bound  {k:34s} {r[k]:.3g}")
    for cache in (_runs, F._mats, F._ints):     # some hundred MB of matrices the later modules have no use for
        cache.clear()


def note(ratios, key, value, bound):
    ratio = value / bound if bound > 0 else (0.0 if value == 0 else np.inf)
    ratios[key] = max(ratios.get(key, 0.0), ratio)
    return ratio


def l2_of(d):
    return np.arange(d) % 5 + 1.0


def assert_persistent(rep, d, what):
    ld = F.round_up(d, 4)
    assert rep["form"] == 1, (what, d, "the persistent route did not run", rep)
    want = F.instance(ld)
    got = {k: rep[k] for k in ("glds", "per", "nblocks", "lds_bytes")}
    assert got == want, (what, d, got, want)


def assert_batched(rep, d, what):
    assert rep["form"] == 0 and rep["nblocks"] == 0, (what, d, rep)


def check_ridge(ratios, key, m, q, rep, w, l2=None, ws=None, rho=RHO, reg=REG, tol=TOL):
    assert rep["status"] == 1, (key, m.d, rep)
    res = float(np.linalg.norm(F.ridge_residual(m, q, rho, reg, w, l2)))
    bound = F.ridge_bound(m, q, rho, reg, tol, rep["iters"], w, l2)
    r = note(ratios, key + " residual", res, bound)
    print(f"{key} d={m.d} iters={rep['iters']} residual {res:.3e} bound {bound:.3e}")
    assert res <= bound, (key, m.d, rep["iters"], res, bound, r)
    if ws is not None:
        err = float(np.linalg.norm(w - ws))
        wb = F.ridge_w_bound(m, q, rho, reg, tol, rep["iters"], w, l2)
        note(ratios, key + " w", err, wb)
        assert err <= wb, (key, m.d, rep["iters"], err, wb)
    return bound


def check_huber(ratios, key, m, q, rep, w, ws=None, rho=RHO, reg=REG, t=T, tol=TOL):
    assert rep["status"] == 1, (key, m.d, rep)
    g = float(np.max(np.abs(F.huber_gradient(m, q, rho, reg, t, w))))
    bound = F.huber_bound(m, q, rho, reg, t, tol, rep["iters"], w)
    r = note(ratios, key + " gradient", g, bound)
    print(f"{key} d={m.d} iters={rep['iters']} phase_a={rep['phase_a']} gradient {g:.3e} bound {bound:.3e}")
    assert g <= bound, (key, m.d, rep["iters"], g, bound, r)
    if ws is not None:
        err = float(np.linalg.norm(w - ws))
        wb = F.huber_w_bound(m, q, rho, reg, t, tol, rep["iters"], w)
        note(ratios, key + " w", err, wb)
        assert err <= wb, (key, m.d, rep["iters"], err, wb)
    return bound


# --------------------------------------------------------------------------------------------------- the entry itself
def test_arguments_are_checked_before_anything_runs(L):
    G, q = np.eye(4), np.ones(4)
    ok = dict(wstep=2, G=G, Q=q, rho=1.0, reg=1.0)
    for bad in (dict(wstep=4), dict(rho=0.0), dict(reg=-1.0), dict(tol=0.0), dict(max_inner=0), dict(route=3),
                dict(route=2, wstep=1), dict(route=2, wstep=3),        # (route 2 is the ridge's: tests/test_gpu_eig.py)
dict(launch_seq0=1 << 20), dict(launch_seq0=-1), dict(l2=-np.ones(4)), dict(l1=np.full(4, np.nan), wstep=1),
                dict(wstep=3, l2=np.ones(4)), dict(wstep=2, two_call=True), dict(wstep=3, rho_dev=True),
                dict(wstep=3, smooth_t=0.0)):
        with pytest.raises(ValueError):
            L.k_wstep_seq(**{**ok, **bad})
    out = L.k_wstep_seq(**ok)
    assert np.allclose(out["w"][0], 0.5, atol=1e-15) and np.all(np.isnan(out["Gw"])) and np.all(np.isnan(out["w_prev"]))


# ------------------------------------------------------------------------------------------------------- exact layer
def run_integer(L, d, route):
    """the three exact fixtures at width d: 0 iterations, w = w0, and (persistent route) G w bit for bit"""
    for name in ("cg", "cg_l2", "ncg"):
        if name == "ncg":
            G, w0, q, Gw = F.integer_huber(d)
            out = L.k_wstep_seq(3, G, q, 1.0, 1.0, w0=w0, smooth_t=0.5, route=route, want_Gw=True)
        else:
            G, w0, q, Gw, l2 = F.integer_ridge(d, l2=name == "cg_l2")
            out = L.k_wstep_seq(2, G, q, 1.0, 1.0, w0=w0, l2=l2, route=route, want_Gw=True)
        rep = out["reports"][0]
        natural_batched = F.instance(F.round_up(d, 4)) is None
        if route == 0 and not natural_batched:
            assert_persistent(rep, d, name)
        else:
            assert_batched(rep, d, name)
        assert rep["status"] == 1 and rep["iters"] == 0, (name, d, rep)
        assert np.array_equal(out["w"][0], w0), (name, d, np.flatnonzero(out["w"][0] != w0)[:8])
        if rep["form"] == 1:
            assert rep["gw_valid"] == 1 and rep["phase_a"] == -1
            got = out["Gw"][0]
            assert np.array_equal(got, Gw.astype(np.float64)), (name, d, np.flatnonzero(got != Gw)[:8])
        else:
            assert rep["gw_valid"] == 0 and np.all(np.isnan(out["Gw"][0]))


@pytest.mark.parametrize("d", F.PERSIST_D)
def test_persistent_exact_integers(L, d):
    """rows, columns, slots (wp_idx), blocks, staging (wp_stage_rows) and the exchange: any mix-up changes an integer"""
    run_integer(L, d, 0)


@pytest.mark.parametrize("d", F.BATCHED_ROUTE1_D + F.BATCHED_NATURAL_D)
def test_batched_exact_integers(L, d):
    run_integer(L, d, 1 if d <= F.WSTEP_PERSIST_MAX_LD else 0)


# ----------------------------------------------------------------------------------------------------- planted layer
_runs = {}


def planted_runs(L, d, route):
    """cold and warm solves of the well-conditioned planted fixtures at width d on one route (shared by the tests below
    and left unchanged): name -> list of (q, w*, w, Gw, report, l2)"""
    key = (d, route)
    if key in _runs:
        return _runs[key]
    m = F.matrix(d, "well")
    rng = np.random.default_rng([d, 53])
    res = {}
    for name in ("cg", "cg_l2", "ncg"):
        l2 = l2_of(d) if name == "cg_l2" else None
        reg = 0.0 if l2 is not None else REG                                   # penalties take the place of reg
        ws, q = F.plant_huber(m, RHO, REG, T) if name == "ncg" else F.plant_ridge(m, RHO, reg, l2)
        q2 = q + 1e-4 * np.max(np.abs(q)) * rng.standard_normal(d)
        kw = dict(rho=RHO, reg=REG, smooth_t=T, tol=TOL, l2=l2, route=route, want_Gw=True)
        wstep = 3 if name == "ncg" else 2
        cold = L.k_wstep_seq(wstep, m.G, q, **kw)
        warm = L.k_wstep_seq(wstep, m.G, np.stack([q2, q]), **kw)              # step 1: q from the solution of q2
        res[name] = [(q, ws, cold["w"][0], cold["Gw"][0], cold["reports"][0], l2),
                     (q2, None, warm["w"][0], warm["Gw"][0], warm["reports"][0], l2),
                     (q, ws, warm["w"][1], warm["Gw"][1], warm["reports"][1], l2)]
    _runs[key] = (m, res)
    return _runs[key]


def check_planted(ratios, route_name, m, res, expect):
    for name, runs in res.items():
        for (q, ws, w, _, rep, l2), start in zip(runs, ("cold", "cold", "warm")):
            expect(rep, m.d, name)
            key = f"{route_name} {name}"
            if name == "ncg":
                check_huber(ratios, key, m, q, rep, w, ws)
            else:
                check_ridge(ratios, key, m, q, rep, w, l2, ws, reg=0.0 if l2 is not None else REG)
        if name != "ncg":   # the warm start solves a right-hand side 1e-4 away: the CG must not need more than from cold
            assert runs[2][4]["iters"] <= runs[0][4]["iters"], (name, m.d, runs[2][4], runs[0][4])


@pytest.mark.parametrize("d", F.PERSIST_D)
def test_persistent_planted_minimisers(L, ratios, d):
    m, res = planted_runs(L, d, 0)
    check_planted(ratios, "persistent", m, res, assert_persistent)


@pytest.mark.parametrize("d", F.PERSIST_D)
def test_persistent_Gw_out_is_G_times_the_returned_w(L, ratios, d):
    """k_cg_persist (with and without the l2 diagonal: the product is with the unshifted G) and k_ncg_persist"""
    m, res = planted_runs(L, d, 0)
    aG = np.abs(m.G)
    for name, runs in res.items():
        for q, ws, w, Gw, rep, l2 in runs:
            assert rep["gw_valid"] == 1 and rep["iters"] > 0, (name, d, rep)
            err = np.abs(Gw - np.asarray(m.mv(w), dtype=np.float64))
            bound = GEMV * (aG @ np.abs(w) + 1)
            note(ratios, f"persistent {name} Gw", float(np.max(err / bound)), 1.0)
            assert np.all(err <= bound), (name, d, float(np.max(err / bound)))


@pytest.mark.parametrize("d", [252, 1100, 2048])
def test_persistent_ill_conditioned_ridge(L, ratios, d):
    """s down to 2^-20: hundreds of exchanges in one launch"""
    m = F.matrix(d, "ill")
    reg = 2.0 ** -20
    ws, q = F.plant_ridge(m, RHO, reg)
    out = L.k_wstep_seq(2, m.G, q, RHO, reg, tol=TOL)
    rep = out["reports"][0]
    assert_persistent(rep, d, "ill")
    assert rep["iters"] >= 100, rep
    check_ridge(ratios, "persistent cg ill", m, q, rep, out["w"][0], None, ws, RHO, reg)


@pytest.mark.parametrize("d", F.BATCHED_ROUTE1_D + F.BATCHED_NATURAL_D)
def test_batched_planted_minimisers(L, ratios, d):
    """k_symv + k_cg_init / k_cg_update (with and without the l2 diagonal) and k_ncg_init / k_ncg_update; below the
    persistent limit the two routes' w agree within the sum of their bounds"""
    natural = d > F.WSTEP_PERSIST_MAX_LD
    m, res = planted_runs(L, d, 0 if natural else 1)
    check_planted(ratios, "batched", m, res, assert_batched)
    if natural:
        return
    _, other = planted_runs(L, d, 0)
    for name in res:
        for a, b in zip(res[name], other[name]):
            (q, _, wa, _, ra, l2), (_, _, wb, _, rb, _) = a, b
            if name == "ncg":
                lim = (np.sqrt(d) * (F.huber_bound(m, q, RHO, REG, T, TOL, ra["iters"], wa)
                                     + F.huber_bound(m, q, RHO, REG, T, TOL, rb["iters"], wb))) / (RHO * m.lam_lo)
            else:
                reg = 0.0 if l2 is not None else REG
                lim = (F.ridge_bound(m, q, RHO, reg, TOL, ra["iters"], wa, l2)
                       + F.ridge_bound(m, q, RHO, reg, TOL, rb["iters"], wb, l2)) / F.a_lo(m, RHO, reg, l2)
            diff = float(np.linalg.norm(wa - wb))
            note(ratios, f"routes agree {name}", diff, lim)
            assert diff <= lim, (name, d, diff, lim)


# -------------------------------------------------------------------------------------------------------------- lasso
KAPPA = 0.75
LASSO_RHO = 0.5                                   # reg = 2 rho kappa


def lasso_case(d, nnz, pen):
    """(m, w*, q, kappa (scalar or vector), shift or None, keyword arguments of the call)"""
    m = F.matrix(d, "well")
    if pen:
        l1 = 2 * LASSO_RHO * (0.25 + (np.arange(d) % 4) / 4.0)       # kappa_j = l1_j / (2 rho) in {1/4, 1/2, 3/4, 1}
        l2 = LASSO_RHO * (np.arange(d) % 3) / 2.0                     # shift_j = l2_j / rho in {0, 1/2, 1}
        kappa, shift = l1 / (2 * LASSO_RHO), l2 / LASSO_RHO
        ws, q, _ = F.plant_lasso(m, kappa, nnz, shift=shift)
        return m, ws, q, kappa, shift, dict(rho=LASSO_RHO, reg=0.0, l1=l1, l2=l2)
    ws, q, _ = F.plant_lasso(m, KAPPA, nnz)
    return m, ws, q, KAPPA, None, dict(rho=LASSO_RHO, reg=2 * LASSO_RHO * KAPPA)


def check_lasso(ratios, key, m, ws, q, kappa, shift, w, rep, unique=True):
    fell = rep["fell_back"] == 1
    # the report is self-consistent: the active-set kernel's status decides the form
    assert rep["fs"][0] in (0, 1, 2) and fell == (rep["fs"][0] != 0) and rep["form"] == (0 if fell else 2), rep
    if not fell:
        assert rep["fs"][3] == np.count_nonzero(w) and rep["iters"] == rep["fs"][1], (rep, np.count_nonzero(w))
    kkt = F.lasso_kkt(m, q, kappa, w, shift)
    bound = F.lasso_bound(m, q, kappa, w, fell)
    r = note(ratios, key + (" fista kkt" if fell else " kkt"), kkt, bound)
    print(f"{key} d={m.d} fs={rep['fs']} fell_back={fell} iters={rep['iters']} kkt {kkt:.3e} bound {bound:.3e}")
    assert kkt <= bound, (key, m.d, rep, kkt, bound, r)
    if ws is not None:
        f, fs = F.lasso_objective(m, q, kappa, w, shift), F.lasso_objective(m, q, kappa, ws, shift)
        assert f <= fs + 1e-10 * abs(fs) + 1e-12, (key, m.d, f, fs)
        if unique:
            lo = m.lam_lo + (float(np.min(shift)) if shift is not None else 0.0)
            err, wb = float(np.linalg.norm(w - ws)), F.lasso_w_bound(m, q, kappa, w, fell, lo)
            note(ratios, key + (" fista w" if fell else " w"), err, wb)
            assert err <= wb, (key, m.d, rep, err, wb)


@pytest.mark.parametrize("pen", [False, True], ids=["scalar", "per_coordinate"])
@pytest.mark.parametrize("d", [300, 2052])
def test_lasso_planted_supports(L, ratios, d, pen):
    """k_lasso_fs with and without per-coordinate penalties on planted supports around its capacity of 96, with G w"""
    aG = None
    for nnz in (1, 8, 64, 96, 97, 200):
        m, ws, q, kappa, shift, kw = lasso_case(d, nnz, pen)
        out = L.k_wstep_seq(1, m.G, q, tol=TOL, want_Gw=True, **kw)
        w, rep = out["w"][0], out["reports"][0]
        check_lasso(ratios, "lasso pen" if pen else "lasso", m, ws, q, kappa, shift, w, rep)
        if nnz <= 64:
            assert rep["form"] == 2 and rep["status"] == 0 and rep["fell_back"] == 0, (nnz, rep)
        if nnz == 200:
            assert rep["form"] == 0 and rep["fell_back"] == 1 and rep["fs"][0] == 1, (nnz, rep)
        assert rep["gw_valid"] == (1 if rep["form"] == 2 else 0)
        if rep["gw_valid"]:
            aG = np.abs(m.G) if aG is None else aG
            err = np.abs(out["Gw"][0] - np.asarray(m.mv(w), dtype=np.float64))      # the unshifted G, also with penalties
            bound = GEMV * (aG @ np.abs(w) + 1)
            note(ratios, ("lasso pen" if pen else "lasso") + " Gw", float(np.max(err / bound)), 1.0)
            assert np.all(err <= bound), (nnz, float(np.max(err / bound)))


@pytest.mark.parametrize("pen", [False, True], ids=["scalar", "per_coordinate"])
def test_lasso_warm_start_beyond_capacity_reports_overflow_first(L, ratios, pen):
    d = 300
    m, ws, q, kappa, shift, kw = lasso_case(d, 8, pen)
    w0 = np.zeros(d)
    w0[::2][:120] = 0.01                                                      # 120 non-zeros > 96
    out = L.k_wstep_seq(1, m.G, q, w0=w0, tol=TOL, want_Gw=True, w_prev=True, **kw)
    rep = out["reports"][0]
    assert rep["fs"] == [1, 0, 0, 120] and rep["fell_back"] == 1 and rep["form"] == 0 and rep["gw_valid"] == 0, rep
    assert np.array_equal(out["w_prev"][0], w0)
    check_lasso(ratios, "lasso overflow", m, ws, q, kappa, shift, out["w"][0], rep)


@pytest.mark.parametrize("pen", [False, True], ids=["scalar", "per_coordinate"])
def test_lasso_call_forms_agree_bit_for_bit(L, pen):
    """rho read on the device, the warm start saved by the kernel, and run_wstep(fs_pending) + finish_wstep_l1 - on a
    support the kernel solves (64) and on one that falls back (200), two steps each so that the second is warm"""
    d = 300
    for nnz in (64, 200):
        m, ws, q, kappa, shift, kw = lasso_case(d, nnz, pen)
        Q = np.stack([q, q + 1e-3])
        w0 = np.where(np.arange(d) % 7 == 0, 0.25, 0.0)
        base = L.k_wstep_seq(1, m.G, Q, w0=w0, tol=TOL, want_Gw=True, **kw)
        for form in (dict(rho_dev=True), dict(two_call=True), dict(w_prev=True), dict(rho_dev=True, w_prev=True)):
            out = L.k_wstep_seq(1, m.G, Q, w0=w0, tol=TOL, want_Gw=True, **kw, **form)
            assert np.array_equal(out["w"], base["w"]), (nnz, form)
            assert np.array_equal(out["Gw"], base["Gw"], equal_nan=True), (nnz, form)
            for a, b in zip(out["reports"], base["reports"]):
                assert {k: a[k] for k in ("form", "status", "iters", "fs", "fell_back", "gw_valid", "last_fista")} == \
                       {k: b[k] for k in ("form", "status", "iters", "fs", "fell_back", "gw_valid", "last_fista")}, (nnz, form)
            if form.get("w_prev"):
                assert np.array_equal(out["w_prev"][0], w0) and np.array_equal(out["w_prev"][1], base["w"][0]), (nnz, form)
            else:
                assert np.all(np.isnan(out["w_prev"]))


def test_lasso_collinear_columns(L, ratios):
    """G = D^T D with two exactly collinear columns: the minimiser need not be unique, the KKT residual and the report
    still have to be right"""
    d = 300
    m, D = F.collinear(d)
    rng = np.random.default_rng(59)
    q = D.T @ rng.standard_normal(D.shape[0])
    for frac in (0.9, 0.5, 0.2):
        kappa = frac * float(np.max(np.abs(q)))
        out = L.k_wstep_seq(1, m.G, q, rho=0.5, reg=kappa, tol=TOL, want_Gw=True)
        check_lasso(ratios, "lasso collinear", m, None, q, kappa, None, out["w"][0], out["reports"][0])


# ---------------------------------------------------------------------------------------------------------- sequences
def expected_launch_seq(seq0, launches):
    s = seq0
    for _ in range(launches):
        s = (s + 1) & 0xfffff
        if s == 0:
            s = 1
    return s


@pytest.mark.parametrize("route", [0, 1], ids=["persistent", "batched"])
@pytest.mark.parametrize("d", F.SEQ_D)
def test_ridge_sequence_on_one_workspace(L, ratios, d, route):
    """uncleared exchange buffers, both parities and the tags of consecutive launches (persistent); batches sized from
    last_iters, with a follow-up batch at the jumps (batched)"""
    m = F.matrix(d, "well")
    _, q0 = F.plant_ridge(m, F.SEQ_RHO, F.SEQ_REG)
    Q = F.drifting_rhs(q0)
    seq0 = 0xffffe if (route == 0 and d == 1028) else 0                      # this one crosses the wrap to 1
    out = L.k_wstep_seq(2, m.G, Q, F.SEQ_RHO, F.SEQ_REG, tol=TOL, route=route, launch_seq0=seq0, want_Gw=True)
    reps = out["reports"]
    for k, rep in enumerate(reps):
        (assert_persistent if route == 0 else assert_batched)(rep, d, f"step {k}")
        check_ridge(ratios, f"sequence {'persistent' if route == 0 else 'batched'} cg", m, Q[k], rep, out["w"][k],
                    rho=F.SEQ_RHO, reg=F.SEQ_REG)
        assert rep["last_iters"] == rep["iters"], (k, rep)
        assert rep["launch_seq"] == (expected_launch_seq(seq0, k + 1) if route == 0 else seq0), (k, rep)
        if k in F.SEQ_JUMPS:
            assert rep["iters"] > reps[k - 1]["last_iters"] + 2, (k, rep, reps[k - 1])
    print(f"d={d} route={route} iters {[r['iters'] for r in reps]}")        # (odd and even: both buffers end a launch)
    if seq0:
        assert [r["launch_seq"] for r in reps[:3]] == [0xfffff, 1, 2]


@pytest.mark.parametrize("route", [0, 1], ids=["persistent", "batched"])
@pytest.mark.parametrize("d", F.SEQ_D)
def test_huber_sequence_on_one_workspace(L, ratios, d, route):
    """the nonlinear CG with its linear first phase: reported pin[2], ncg_skip and ncg_backoff follow run_ncg_persist's
    rule - accepted: back-off 0; dropped: pauses of 1, 2, 4 ... 16 w-steps; a paused step does not try"""
    m = F.matrix(d, "well")
    _, q0 = F.plant_huber(m, RHO, REG, T)
    Q = F.drifting_rhs(q0)
    seq0 = 0xffffe if (route == 0 and d == 20) else 0
    out = L.k_wstep_seq(3, m.G, Q, RHO, REG, smooth_t=T, tol=TOL, route=route, launch_seq0=seq0, want_Gw=True)
    reps = out["reports"]
    skip = backoff = 0
    tried = 0
    for k, rep in enumerate(reps):
        (assert_persistent if route == 0 else assert_batched)(rep, d, f"step {k}")
        check_huber(ratios, f"sequence {'persistent' if route == 0 else 'batched'} ncg", m, Q[k], rep, out["w"][k])
        assert rep["last_fista"] == rep["iters"], (k, rep)
        if route == 1:
            assert rep["phase_a"] == -1 and rep["ncg_skip"] == 0 and rep["ncg_backoff"] == 0 and rep["launch_seq"] == 0
            continue
        assert rep["launch_seq"] == expected_launch_seq(seq0, k + 1), (k, rep)
        if skip > 0:
            assert rep["phase_a"] == -1, (k, "a paused step tried the linear phase", rep)
        if rep["phase_a"] == 1:
            backoff = 0
        elif rep["phase_a"] == 0:
            backoff = min(2 * backoff, 16) if backoff else 1
            skip = backoff
        elif skip > 0:
            skip -= 1
        tried += rep["phase_a"] != -1
        assert (rep["ncg_skip"], rep["ncg_backoff"]) == (skip, backoff), (k, rep, skip, backoff)
    if route == 0:
        assert reps[0]["phase_a"] != -1 and tried >= 1, reps[0]             # the first step is neither paused nor done on entry
        print(f"d={d} phase_a per step: {[r['phase_a'] for r in reps]} iters {[r['iters'] for r in reps]}")
