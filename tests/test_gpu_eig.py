"""The eigendecomposition ridge (csrc/eig.hip: k_eig_init, k_eig_step, k_eig_finish, k_eig_coef, k_eig_apply) on prescribed
G and q.  Two ways in: rbl_k_eig runs launch_eig_jacobi alone and returns the basis; rbl_k_wstep_seq with route 2
decomposes once on the workspace as rbl_gram_finish does and runs K w-steps through run_wstep (form 3).  Fixtures, bounds
and the restatement's figures: tests/wstep_fixtures.py and tests/eig_ref.py, checked on the CPU by tests/test_eig_host.py.
  decomposition  V = Vt^T bit for bit, identity padding, lambda >= 0, orthogonality and eigen-residual in longdouble
                 through Mat.mv, eigenvalues against numpy.linalg.eigvalsh, exact matrices, two calls bit for bit
  contract       sweeps >= 1 where the restatement converges; sweeps == 0 and ld > 2048 keep the CG and meet its bound
  ridge          planted minimisers at four (rho, reg), 3 drifting right-hand sides on one workspace: form 3, iters 1,
                 the true residual within ridge_bound(tol = 1e-13, iters = 2); reg = 0 beside the CG
  handle         one child process under RBL_RIDGE_EIG=1: owner and borrower, an l1 owner, rbl_set_penalty, a padded
                 width with a tiny reg (l2_reg = 0 is rejected by rbl_create: reg == 0 is a kernel-level case only)
W comes back as K x d: the padding of w is not visible through the entry.  It is zero because the padding rows and
columns of Vt and V are the identity with lambda = 0 (asserted here) and q is zero there; tests/test_eig_host.py asserts
w[d:] == 0 on the restatement.
Every test prints its largest error / bound before it asserts (pytest -s).

Measured on an MI355X when this module was written (largest error / bound per family):
  decomposition   orthogonality: well 0.094, ill 0.245, collinear 0.135, rank one 0.017; eigen-residual: well 0.0075,
                  ill 0.021, collinear 0.249, rank one 0.0018; exact matrices 0.  Sweeps equal the restatement's on every
                  fixture but two (ill d = 65: 19 against 18, ill d = 132: 26 against 27); ill d = 257 stops at the cap
                  on both (sweeps 0, the CG runs: 0.058).  d = 2048: 6 sweeps, 0.36 s with the copies.
  ridge, residual with one refinement step (as first shipped) -> with two:
                  collinear, first right-hand side, rho = 217 d, reg = 1e-4: 11.7 (d = 63), 7.3 (64), 5.65 (65),
                  4.7 (256), 1.13 (260) -> at most 0.05 over all steps; rho = 217 d, reg = 0.01: 5.65 (d = 255) -> 0.0021;
                  collinear at rho = 1 and 2^-12: 0.0014 / 0.0007 -> 0.0018 / 0.0007; well and ill, all four pairs:
                  0.0007 - 0.0025 before and after
  reg = 0         as first shipped NaN in all of w (well, d = 63); now 0.0014 (well and collinear), the CG 0.54 / 0.067
Deliberately wrong kernels, each tried once: without the Vt rotation in k_eig_step test_decomposition, test_exact_matrices,
test_ridge_planted_minimisers and test_ridge_without_regulariser fail; with lane stride 32 in k_eig_apply the last two
(every width from 63 up); without the refinement test_ridge_planted_minimisers on collinear and at d = 1000."""
import gc
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import wstep_fixtures as F

pytestmark = pytest.mark.gpu

TOL = 1e-13                       # the handle's own default w_tol
LD = F.LD
WIDE = [("well", d) for d in F.EIG_WIDE_D]
SAMPLE = 64                       # rows held to the longdouble measures where d > 300 (all of them below)


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    gc.collect()
    return rbl._lib


@pytest.fixture(scope="module")
def ratios():
    """largest error / bound per family, printed when the module ends (pytest -s)"""
    r = {}
    yield r
    for k in sorted(r):
        print(f"eig error/bound  {k:44s} {r[k]:.3g}")
    for cache in (_decs, F._mats):
        cache.clear()


def note(ratios, key, value, bound):
    ratio = value / bound if bound > 0 else (0.0 if value == 0 else np.inf)
    ratios[key] = max(ratios.get(key, 0.0), ratio)
    return ratio


def case_id(c):
    return f"{c[0]}-{c[1]}"


_decs = {}


def device_dec(L, kind, d):
    """(Mat, the device's decomposition, seconds) of one fixture: computed once, shared by the tests, left unchanged"""
    key = (kind, d)
    if key not in _decs:
        m = F.eig_matrix(kind, d)
        t0 = time.perf_counter()
        dec = L.k_eig(m.G)
        _decs[key] = (m, dec, time.perf_counter() - t0)
    return _decs[key]


def rows_to_check(d):
    return np.arange(d) if d <= 300 else np.sort(np.random.default_rng([d, 61]).choice(d, SAMPLE, replace=False))


def orthogonality(Vt, rows):
    V = Vt.astype(LD)
    return float(np.max(np.abs(V[rows] @ V.T - np.eye(V.shape[0], dtype=LD)[rows])))


def eigen_residual(m, Vt, lam, rows):
    worst = 0.0
    for j in rows:
        v = Vt[j, :m.d].astype(LD)
        r = m.mv(v) - LD(lam[j]) * v
        worst = max(worst, float(np.sqrt(np.sum(r * r))))
    return worst


# ------------------------------------------------------------------------------------------------------ the entries
def test_arguments_are_checked_before_anything_runs(L):
    G, q = np.eye(4), np.ones(4)
    with pytest.raises(ValueError):
        L.k_eig(np.eye(F.EIG_BEYOND_D))                            # beyond the width the solver decomposes
    with pytest.raises(ValueError):
        L.k_eig(np.ones((3, 4)))
    for wstep in (1, 3):                                           # route 2 is the ridge's
        with pytest.raises(ValueError):
            L.k_wstep_seq(wstep, G, q, 1.0, 1.0, route=2)
    for bad in (dict(route=3), dict(route=-1)):
        with pytest.raises(ValueError):
            L.k_wstep_seq(2, G, q, 1.0, 1.0, **bad)
    out = L.k_wstep_seq(2, G, q, 1.0, 1.0, route=2)
    assert out["reports"][0]["form"] == 3 and out["reports"][0]["iters"] == 1
    assert np.array_equal(out["w"][0], np.full(4, 0.5))           # (G + I) w = q in the basis V = I: exact
    # per-coordinate penalties are no multiple of the identity: route 2 decomposes and the CG still runs
    out = L.k_wstep_seq(2, G, q, 1.0, 0.0, l2=np.ones(4), route=2)
    assert out["reports"][0]["form"] in (0, 1) and np.allclose(out["w"][0], 0.5, atol=1e-15)


# ---------------------------------------------------------------------------------------------------- decomposition
@pytest.mark.parametrize("case", F.EIG_CASES + WIDE, ids=case_id)
def test_decomposition(L, ratios, case):
    kind, d = case
    m, dec, secs = device_dec(L, kind, d)
    ld, Vt, V, lam = dec["ld"], dec["Vt"], dec["V"], dec["lam"]
    ref = F.EIG_REF_SWEEPS[case]
    print(f"{kind} d={d} ld={ld} sweeps: device {dec['sweeps']}  restatement {ref}  ({secs:.2f} s with the copies)")
    assert ld == F.round_up(d, 4) and Vt.shape == (ld, ld)
    assert 1 <= dec["sweeps"] <= 30, (case, dec["sweeps"])         # the restatement converges on every one of these
    assert np.array_equal(V, Vt.T), case                           # bit for bit
    eye = np.eye(ld)
    assert np.array_equal(Vt[d:], eye[d:]) and np.array_equal(Vt[:, d:], eye[:, d:]), case
    assert np.array_equal(lam[d:], np.zeros(ld - d)) and np.all(lam >= 0.0) and np.all(np.isfinite(Vt)), case
    rows = rows_to_check(d)
    orth, ob = orthogonality(Vt, rows), F.eig_orth_bound(d)
    r1 = note(ratios, f"{kind} orthogonality", orth, ob)
    print(f"{kind} d={d} max |V^T V - I| {orth:.3e} bound {ob:.3e} ratio {r1:.3g}")
    assert orth <= ob, (case, orth, ob)
    if kind == "zero":
        return                                                     # (lam_hi = 0: test_exact_matrices holds lambda to 0)
    res, rb = eigen_residual(m, Vt, lam, rows), F.eig_res_bound(m)
    r2 = note(ratios, f"{kind} eigen-residual", res, rb)
    ev = np.linalg.eigvalsh(m.G)
    dev = float(np.max(np.abs(np.sort(lam[:d]) - ev)))
    r3 = note(ratios, f"{kind} eigenvalues", dev, rb)
    print(f"{kind} d={d} max ||G v - lambda v|| {res:.3e} |lambda - eigvalsh| {dev:.3e} bound {rb:.3e} ratios {r2:.3g} {r3:.3g}")
    assert res <= rb, (case, res, rb)
    assert dev <= rb, (case, dev, rb)


def test_widest_decomposition_is_timed(L):
    """d = 2048, the limit of the route (the time includes the copies of G, Vt and V: 100 MB)"""
    _, dec, secs = device_dec(L, "well", F.EIG_MAX_LD)
    print(f"d = {F.EIG_MAX_LD}: {dec['sweeps']} sweeps in {secs:.2f} s")
    assert dec["sweeps"] >= 1 and secs <= 10.0, secs


@pytest.mark.parametrize("d", F.EIG_WIDTHS)
def test_exact_matrices(L, d):
    """c I and a diagonal G: nothing to rotate, one sweep, V = I and lambda = the diagonal, exactly; G = 0: lambda = 0;
    rows of G that are zero from the start stay unit vectors in Vt and V, with lambda = 0"""
    for kind in F.EIG_EXACT:
        m, dec, _ = device_dec(L, kind, d)
        ld, Vt, V, lam = dec["ld"], dec["Vt"], dec["V"], dec["lam"]
        eye = np.eye(ld)
        if kind != "rankone":
            assert dec["sweeps"] == 1, (kind, d, dec["sweeps"])
            assert np.array_equal(Vt, eye) and np.array_equal(V, eye), (kind, d)
            assert np.array_equal(lam[:d], np.diag(m.G)) and np.array_equal(lam[d:], np.zeros(ld - d)), (kind, d)
        null = F.eig_null_rows(kind, d)
        assert np.array_equal(Vt[null], eye[null]) and np.array_equal(Vt[:, null], eye[:, null]), (kind, d)
        assert np.array_equal(V[null], eye[null]) and np.array_equal(lam[null], np.zeros(null.size)), (kind, d)
        if kind == "rankone":
            u = m._B[0]
            top = float(u @ u)
            srt = np.sort(lam[:d])
            assert abs(srt[-1] - top) <= F.eig_res_bound(m) and np.all(srt[:-1] <= F.eig_res_bound(m)), (d, srt[-3:], top)


@pytest.mark.parametrize("case", [("well", 65), ("ill", 132), ("collinear", 257), ("rankone", 260)], ids=case_id)
def test_two_calls_agree_bit_for_bit(L, case):
    """ranks that each decompose the same G must hold the same basis"""
    m, a, _ = device_dec(L, *case)
    b = L.k_eig(m.G)
    assert a["sweeps"] == b["sweeps"]
    for k in ("Vt", "V", "lam"):
        assert np.array_equal(a[k], b[k]), (case, k)


# ------------------------------------------------------------------------------------------------- ridge, route 2
def rho_label(rho):
    return "217d" if rho > 100 else f"{rho:g}"


def run_route2(L, ratios, m, rho, reg, K=3):
    ws, q0 = F.plant_ridge(m, rho, reg)
    Q = F.eig_drift(m, q0, K)
    out = L.k_wstep_seq(2, m.G, Q, rho, reg, tol=TOL, route=2)
    for k, rep in enumerate(out["reports"]):
        assert rep["form"] == 3 and rep["iters"] == 1, (m.kind, m.d, k, rep)
        check_ridge(ratios, f"route 2 {m.kind} rho={rho_label(rho)} reg={reg:g}", m, Q[k], rho, reg, out["w"][k], 2,
                    ws if k == 0 else None)
    return out


def check_ridge(ratios, key, m, q, rho, reg, w, iters, ws=None):
    assert np.all(np.isfinite(w)), (key, m.d, rho, reg)
    res = float(np.linalg.norm(F.ridge_residual(m, q, rho, reg, w)))
    bound = F.ridge_bound(m, q, rho, reg, TOL, iters, w)
    r = note(ratios, key + " residual", res, bound)
    print(f"{key} d={m.d} iters={iters} residual {res:.3e} bound {bound:.3e} ratio {r:.3g}")
    assert res <= bound, (key, m.d, rho, reg, res, bound, r)
    if ws is not None and m.lam_lo > 0:
        err, wb = float(np.linalg.norm(w - ws)), F.ridge_w_bound(m, q, rho, reg, TOL, iters, w)
        note(ratios, key + " w", err, wb)
        assert err <= wb, (key, m.d, rho, reg, err, wb)


@pytest.mark.parametrize("case", F.EIG_RIDGE_CASES + WIDE[:1], ids=case_id)
def test_ridge_planted_minimisers(L, ratios, case):
    """(rho G + reg I) w = rho q through the basis and its refinement against G: 3 drifting right-hand sides on one
    workspace at each (rho, reg); iters = 2 in the bound stands for the two applications of the basis"""
    m = F.eig_matrix(*case)
    for rho, reg in F.eig_rho_reg(m.d):
        run_route2(L, ratios, m, rho, reg)


@pytest.mark.parametrize("case", [("well", 63), ("collinear", 64)], ids=case_id)
def test_ridge_without_regulariser(L, ratios, case):
    """reg = 0: rho lambda + reg is exactly 0 on the padding rows (d = 63) and at rounding level on the null row of the
    collinear matrix: w stays finite and meets the bound, as the CG (route 0) does on the same input.  The right-hand
    sides stay in range(G) (F.eig_drift): with reg = 0 a singular system has a solution only there."""
    m = F.eig_matrix(*case)
    rho = 1.0
    ws, q0 = F.plant_ridge(m, rho, 0.0)
    Q = F.eig_drift(m, q0)
    cg = L.k_wstep_seq(2, m.G, Q, rho, 0.0, tol=TOL, route=0)
    for k, rep in enumerate(cg["reports"]):
        assert rep["form"] == 1 and rep["status"] == 1, rep
        check_ridge(ratios, f"reg=0 {m.kind} route 0", m, Q[k], rho, 0.0, cg["w"][k], rep["iters"], ws if k == 0 else None)
    out = L.k_wstep_seq(2, m.G, Q, rho, 0.0, tol=TOL, route=2)
    for k, rep in enumerate(out["reports"]):
        assert rep["form"] == 3 and rep["iters"] == 1, rep
        check_ridge(ratios, f"reg=0 {m.kind} route 2", m, Q[k], rho, 0.0, out["w"][k], 2, ws if k == 0 else None)


# ---------------------------------------------------------------------------------------------- convergence contract
def test_unconverged_decomposition_keeps_the_cg(L, ratios):
    """"ill" at d = 257: the restatement is not through after 30 sweeps.  Whatever the device reports, the contract
    holds: sweeps == 0 means route 2 runs a CG form and meets the CG's bound, sweeps > 0 means form 3"""
    d = F.EIG_ILL_STALLS_D
    m = F.matrix(d, "ill")
    dec = L.k_eig(m.G)
    print(f"ill d={d} sweeps: device {dec['sweeps']}  restatement 0 (not converged)")
    assert 0 <= dec["sweeps"] <= 30
    eye = np.eye(dec["ld"])
    assert np.array_equal(dec["Vt"][d:], eye[d:]) and np.array_equal(dec["Vt"][:, d:], eye[:, d:])
    if dec["sweeps"] == 0:
        assert np.all(np.isnan(dec["V"])) and np.all(np.isnan(dec["lam"]))      # only a converged run writes them
    rho, reg = 1.0, 2.0 ** -20
    ws, q = F.plant_ridge(m, rho, reg)
    out = L.k_wstep_seq(2, m.G, np.stack([q, q + 1e-3]), rho, reg, tol=TOL, route=2)
    for k, rep in enumerate(out["reports"]):
        qk = q if k == 0 else q + 1e-3
        if dec["sweeps"] == 0:
            assert rep["form"] in (0, 1) and rep["status"] == 1 and rep["iters"] > 1, rep
            check_ridge(ratios, "unconverged: cg", m, qk, rho, reg, out["w"][k], rep["iters"], ws if k == 0 else None)
        else:
            assert rep["form"] == 3 and rep["iters"] == 1, rep
            check_ridge(ratios, "ill 257 route 2", m, qk, rho, reg, out["w"][k], 2, ws if k == 0 else None)


def test_beyond_the_limit_the_cg_runs(L, ratios):
    """ld = 2052 > 2048: no decomposition, form is never 3"""
    d = F.EIG_BEYOND_D
    m = F.matrix(d, "well")
    ws, q = F.plant_ridge(m, 1.0, 0.5)
    out = L.k_wstep_seq(2, m.G, np.stack([q, q + 1e-3]), 1.0, 0.5, tol=TOL, route=2)
    for k, rep in enumerate(out["reports"]):
        assert rep["form"] == 0 and rep["status"] == 1 and rep["iters"] > 1, rep
        check_ridge(ratios, "beyond the limit: cg", m, q if k == 0 else q + 1e-3, 1.0, 0.5, out["w"][k], rep["iters"],
                    ws if k == 0 else None)


# ------------------------------------------------------------------------------------------------------ handle level
CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import admm_for_rank_based_loss_amd as R
from oracle import problems, admm

NIT = 8


def run(h, ref_tol, form3, what):
    ref, tol = ref_tol                 # the tolerances of test_gpu_solver.py::test_ridge_by_eigendecomposition_variant
    s = h._s
    P, Dl = [], []
    for i in range(NIT):
        st = s.step(True)
        assert (st.wstep_form == 3) == form3, (what, i, st.wstep_form)
        assert not form3 or st.inner_iters == 1, (what, i, st.inner_iters)
        assert np.isfinite(st.primal) and np.isfinite(st.dual), (what, i)
        assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (what, i, st.primal, ref.primal[i])
        assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), (what, i, st.dual, ref.dual[i])
        P.append(st.primal), Dl.append(st.dual)
    w = s.get_state()['w']
    assert np.all(np.isfinite(w)), what
    assert np.max(np.abs(w - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w))), (what, np.max(np.abs(w - ref.w)))
    return np.array(P), np.array(Dl), w


def oracle(X, y, kw):
    ref = admm.admm_solve(X, y, max_iter=NIT, mode='exact', tol=0.0, **kw)
    return ref, (1e-9 if kw['loss'] == 'binary_cross_entropy' else 1e-7)


def make(X, y, kw, share=None):
    return R.ADMMmethod(X, y, max_iter=NIT, tol=0.0, storage='f64', share_data=share, **kw)


X, y = problems.make_problem(1200, 65, seed=7)
A = dict(weight_function='erm', loss='hinge', l2_reg=0.01)
B = dict(weight_function='superquantile', loss='binary_cross_entropy', l2_reg=1e-3, args=[0.5])
C = dict(weight_function='erm', loss='binary_cross_entropy', l1_reg=0.01)
refA, refB = oracle(X, y, A), oracle(X, y, B)

# an l2 owner and a borrower with another reg: both through the basis, and as each runs alone
own = make(X, y, A)
bor = make(X, y, B, share=own)
ra, rb = run(own, refA, True, 'owner'), run(bor, refB, True, 'borrower')
sa, sb = run(make(X, y, A), refA, True, 'owner alone'), run(make(X, y, B), refB, True, 'borrower alone')
for got, alone, what in ((ra, sa, 'owner'), (rb, sb, 'borrower')):
    for g, a in zip(got, alone):
        assert np.allclose(g, a, rtol=1e-12, atol=1e-14), (what, np.max(np.abs(g - a)))
del own, bor

# an l1 owner decomposes nothing: its l2 borrower runs the CG
own = make(X, y, C)
bor = make(X, y, A, share=own)
run(bor, refA, False, 'l2 borrower of an l1 owner')
del own, bor

# per-coordinate penalties are no multiple of the identity: the handle leaves form 3 (l2_j = reg is the same problem)
h = make(X, y, A)
h._s.set_penalty(l2=np.full(65, 0.01))
run(h, refA, False, 'set_penalty')
del h

# l2_reg = 0 never reaches the basis through a handle: rbl_create asks for reg > 0 (reg == 0 is the kernel-level tests')
X0, y0 = problems.make_problem(900, 63, seed=9)
try:
    make(X0, y0, dict(weight_function='erm', loss='binary_cross_entropy', l2_reg=0.0))
    raise SystemExit('l2_reg = 0.0 was accepted')
except ValueError as e:
    assert 'positive' in str(e), e
# the smallest reg at a padded width instead
Z = dict(weight_function='erm', loss='binary_cross_entropy', l2_reg=1e-8)
run(make(X0, y0, Z), oracle(X0, y0, Z), True, 'l2_reg = 1e-8')
print('OK')
"""


def test_handles_under_the_environment_switch():
    """RBL_RIDGE_EIG=1 is read once per process: one child runs every handle-level case"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", CHILD % root], env=dict(os.environ, RBL_RIDGE_EIG="1"), capture_output=True,
                         text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-500:], out.stderr[-3000:])
