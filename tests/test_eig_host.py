"""csrc/eig.hip on the CPU: the pair schedule as an exact integer property, the new exact fixtures, and the NumPy
restatement (tests/eig_ref.py) run over the fixture list of tests/wstep_fixtures.py - the sweeps, orthogonality,
eigen-residual and ridge residual it reaches are what the two constants EIG_ORTH_K and EIG_RES_K and the recorded sweep
counts of the GPU tests stand on.  No GPU and no library call."""
import itertools

import numpy as np
import pytest

import eig_ref as E
import wstep_fixtures as F

LD = F.LD


# ------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("m", list(range(2, 67, 2)) + [258, 1000])
def test_every_pair_of_players_meets_exactly_once_per_sweep(m):
    seen = np.zeros((m, m), dtype=np.int64)
    for r in range(m - 1):
        p, q = E.pairs(m, r)
        assert p.size == m // 2 and np.all(p < q) and np.all(p >= 0) and np.all(q < m)
        assert np.unique(np.concatenate([p, q])).size == m          # the pairs of a round are disjoint: every player once
        np.add.at(seen, (p, q), 1)
    want = np.triu(np.ones((m, m), dtype=np.int64), 1)
    assert np.array_equal(seen, want)


@pytest.mark.parametrize("d", [1, 3, 5, 63, 65, 257])
def test_an_odd_width_meets_the_dummy_once_per_round_and_skips_it(d):
    m = E.players(d)
    assert m == d + 1
    ld = E.round_up(d, 4)
    for r in range(m - 1):
        p, q = E.pairs(m, r)
        assert np.count_nonzero(q == d) == 1 and np.all(p < d)     # the dummy is index d, always the larger of its pair
    # the step leaves the dummy's row (a padding row of the ld x ld arrays) alone: marked rows stay bit for bit
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d))
    Bt, Vt = np.zeros((ld, ld)), np.eye(ld)
    Bt[:d, :d] = A @ A.T
    Bt[d:], Vt[d:] = 7.0, 9.0                                       # (never rows of a real problem: a rotation would mix them in)
    for r in range(m - 1):
        E.step(Bt, Vt, d, m, r, 0.0)
    assert np.all(Bt[d:] == 7.0) and np.all(Vt[d:] == 9.0)
    assert np.all(np.isfinite(Bt[:d])) and np.all(np.isfinite(Vt[:d]))


def test_even_widths_have_no_dummy():
    for d in (2, 64, 256, 260):
        m = E.players(d)
        assert m == d
        for r in range(m - 1):
            p, q = E.pairs(m, r)
            assert np.all(q < d)


# ------------------------------------------------------------------------------------------------------- fixtures
def test_fixture_list_covers_the_widths():
    assert F.EIG_WIDTHS == [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 260]
    assert all(d <= 132 for d in F.EIG_ILL_D) and F.EIG_ILL_STALLS_D == 257
    assert F.EIG_WIDE_D == [1000, 2048] and F.EIG_BEYOND_D == F.EIG_MAX_LD + 4
    assert set(F.EIG_REF_SWEEPS) == set(F.EIG_CASES) | {("well", d) for d in F.EIG_WIDE_D}
    assert [(rho, reg) for rho, reg in F.eig_rho_reg(10)] == [(1.0, 0.5), (2.0 ** -12, 0.5), (2170.0, 0.01), (2170.0, 1e-4)]


@pytest.mark.parametrize("kind", F.EIG_EXACT)
def test_exact_matrices_are_their_factors(kind):
    for d in F.EIG_WIDTHS:
        m = F.eig_matrix(kind, d)
        assert np.array_equal(m.G, m.G.T) and m.G.shape == (d, d)
        full = np.diag(m._s) + m._B.T @ m._B                        # longdouble
        assert np.array_equal(m.G.astype(LD), full), (kind, d)
        w = np.random.default_rng(d).standard_normal(d)
        assert np.allclose(np.asarray(m.mv(w), dtype=np.float64), m.G @ w, rtol=0, atol=1e-12 * (1 + m.lam_hi))
        ev = np.linalg.eigvalsh(m.G)
        assert ev[0] >= m.lam_lo - 1e-12 * (1 + m.lam_hi) and ev[-1] <= m.lam_hi * (1 + 1e-12), (kind, d)
        null = F.eig_null_rows(kind, d)
        assert np.all(m.G[null] == 0.0) and np.all(m.G[:, null] == 0.0)
        if kind == "diagzero":
            assert null.size == 1 and m.G[d // 2, d // 2] == 0.0
        if kind == "rankone" and d >= 3:
            assert null.size >= 1 and np.linalg.matrix_rank(m.G) == 1


def test_drift_on_a_singular_matrix_stays_in_range():
    """collinear(d): column 5 = 2 col 3 - col 4, so n = e5 - 2 e3 + e4 spans the null space; every right-hand side of
    eig_drift is orthogonal to it up to the rounding of q, while drifting_rhs itself is not (1e-3 per step)"""
    for d in (64, 257):
        m = F.eig_matrix("collinear", d)
        n = np.zeros(d)
        n[[5, 3, 4]] = 1.0, -2.0, 1.0
        assert np.all(m.G @ n == 0.0)
        _, q0 = F.plant_ridge(m, 1.0, 0.0)
        Q = F.eig_drift(m, q0)
        assert Q.shape == (3, d) and np.array_equal(Q[0], q0)
        assert np.all(np.abs(Q @ n) <= 8 * F.EPS * np.linalg.norm(Q, axis=1) * np.linalg.norm(n))
        step = np.linalg.norm(Q[1:] - Q[:-1], axis=1) / np.sqrt(d)
        assert np.all(np.abs(step - 1e-3) <= 1e-6)                   # unit-RMS directions times 1e-3 (q itself is ~1e3)
        assert np.max(np.abs(F.drifting_rhs(q0, K=3, jumps=()) @ n)) > 1e-4
    m = F.matrix(64, "well")
    _, q0 = F.plant_ridge(m, 1.0, 0.5)
    assert np.array_equal(F.eig_drift(m, q0), F.drifting_rhs(q0, K=3, jumps=()))


# ---------------------------------------------------------------------------------------------------- restatement
_table = {}


def restated(case):
    """dict(sweeps, orth, res (both in units of d eps; res also over lam_hi), dec, m) of one fixture, computed once"""
    if case not in _table:
        m = F.eig_matrix(*case)
        dec = E.jacobi(m.G)
        row = dict(m=m, dec=dec, sweeps=dec["sweeps"])
        if dec["sweeps"]:
            row["orth"] = E.orthogonality(dec["Vt"]) / (m.d * F.EPS)
            row["res"] = E.eigen_residual(m, dec["Vt"], dec["lam"]) / (m.d * F.EPS * m.lam_hi) if m.lam_hi > 0 else 0.0
        _table[case] = row
    return _table[case]


@pytest.mark.parametrize("case", F.EIG_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_restatement_decomposes_every_fixture(case):
    """the reference for EIG_ORTH_K and EIG_RES_K (4 x the largest value here): every fixture stays within half its
    bound, i.e. the constants are at least twice what the restatement needs on this machine's NumPy"""
    kind, d = case
    row = restated(case)
    dec, m = row["dec"], row["m"]
    assert 1 <= row["sweeps"] <= E.SWEEP_CAP
    assert abs(row["sweeps"] - F.EIG_REF_SWEEPS[case]) <= 1, (case, row["sweeps"])     # (another NumPy may sum in another order)
    print(f"{kind:10s} d={d:4d} sweeps {row['sweeps']:2d} orthogonality {row['orth']:.3f} d eps  residual {row['res']:.3f} d eps")
    ld = dec["ld"]
    eye = np.eye(ld)
    assert np.array_equal(dec["V"], dec["Vt"].T)
    assert np.array_equal(dec["Vt"][d:], eye[d:]) and np.array_equal(dec["Vt"][:, d:], eye[:, d:])
    assert np.all(dec["lam"] >= 0) and np.all(dec["lam"][d:] == 0)
    assert row["orth"] <= F.EIG_ORTH_K / 2 and row["res"] <= F.EIG_RES_K / 2, (case, row["orth"], row["res"])
    if m.lam_hi > 0:
        ev = np.linalg.eigvalsh(m.G)
        assert np.max(np.abs(np.sort(dec["lam"][:d]) - ev)) <= F.eig_res_bound(m) / 2
    null = F.eig_null_rows(kind, d)
    assert np.array_equal(dec["Vt"][null], eye[null]) and np.all(dec["lam"][null] == 0)
    if kind in ("identity", "diagzero", "zero"):
        assert row["sweeps"] == 1 and np.array_equal(dec["Vt"], eye) and np.array_equal(dec["lam"][:d], np.diag(m.G))


def test_constants_are_four_times_the_restatement():
    """K = 4 x the largest restatement value, rounded up: not below it, and not more than 4.5 x it"""
    rows = [restated(c) for c in F.EIG_CASES]
    orth = max([r["orth"] for r in rows] + [v[1] for v in F.EIG_REF_WIDE.values()])
    res = max([r["res"] for r in rows] + [v[2] for v in F.EIG_REF_WIDE.values()])
    print(f"largest orthogonality {orth:.3f} d eps, largest residual {res:.3f} d eps")
    assert 3.5 * orth <= F.EIG_ORTH_K <= 4.5 * orth and 3.5 * res <= F.EIG_RES_K <= 4.5 * res, (orth, res)


def test_ill_at_257_does_not_converge_within_the_cap():
    """six clustered levels over eight decades: |cos| stays near 0.8 for a dozen sweeps and 30 do not suffice - the
    caller is to keep the CG (sweeps == 0, no V, no lambda)"""
    trace = []
    dec = E.jacobi(F.matrix(F.EIG_ILL_STALLS_D, "ill").G, trace=trace)
    print("largest |cos| per sweep:", " ".join(f"{t:.1e}" for t in trace))
    assert dec["sweeps"] == 0 and dec["V"] is None and dec["lam"] is None and len(trace) == E.SWEEP_CAP
    assert trace[-1] > E.OFF_STOP and sum(t > 0.5 for t in trace) >= 8


@pytest.mark.parametrize("case", F.EIG_RIDGE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_restated_ridge_meets_the_bound_with_two_refinements(case):
    """launch_ridge_eig as shipped (two refinement steps) within ridge_bound(tol = 1e-13, iters = 2) at every (rho, reg),
    with room (a tenth of the bound); one refinement is printed beside it - on the collinear matrices at the rho cap
    with reg = 1e-4 it misses the bound by one to two orders, which is why there are two.  Padding of w stays zero."""
    row = restated(case)
    m, dec = row["m"], row["dec"]
    d = m.d
    Gp = E.pad(m.G)
    for rho, reg in F.eig_rho_reg(d):
        ws, q = F.plant_ridge(m, rho, reg)
        _, qp = E.pad(m.G, q)
        ratio = {}
        for nref in (1, 2):
            w = E.ridge(Gp, dec, qp, rho, reg, nref)
            assert np.all(w[d:] == 0.0), (case, rho, reg)
            res = float(np.linalg.norm(F.ridge_residual(m, q, rho, reg, w[:d])))
            ratio[nref] = res / F.ridge_bound(m, q, rho, reg, 1e-13, 2, w[:d])
        print(f"{case[0]:10s} d={d:4d} rho={rho:<10g} reg={reg:<7g} residual / bound: one refinement {ratio[1]:.3g}, two {ratio[2]:.3g}")
        assert ratio[2] <= 0.1, (case, rho, reg, ratio)
        for k, qk in enumerate(F.eig_drift(m, q)[1:], 1):           # the later right-hand sides of the GPU test's sequence
            w = E.ridge(Gp, dec, E.pad(m.G, qk)[1], rho, reg, 2)[:d]
            res = float(np.linalg.norm(F.ridge_residual(m, qk, rho, reg, w)))
            assert res <= 0.1 * F.ridge_bound(m, qk, rho, reg, 1e-13, 2, w), (case, rho, reg, k)
        if m.lam_lo > 0:
            err = float(np.linalg.norm(E.ridge(Gp, dec, qp, rho, reg, 2)[:d] - ws))
            assert err <= F.ridge_w_bound(m, q, rho, reg, 1e-13, 2, ws), (case, rho, reg, err)


@pytest.mark.parametrize("case", [("well", 63), ("collinear", 64)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_restated_ridge_without_regulariser(case):
    """reg = 0: the plain quotient is 0 / 0 on the padding row (d = 63) and spreads NaN over all of w; on the collinear
    matrix the null row's Rayleigh quotient is rounding level, not 0 (1e-13 here), and the plain quotient puts 1e4 ||w||
    into the null space - a true residual of 200 x the bound and more.  With the coefficient 0 on the rows of the null
    space w is finite, zero on the padding, and within the bound."""
    row = restated(case)
    m, dec = row["m"], row["dec"]
    d = m.d
    ws, q = F.plant_ridge(m, 1.0, 0.0)
    Gp, qp = E.pad(m.G, q)
    print(f"{case[0]} d={d} smallest lambda {np.sort(dec['lam'])[:2]}")
    plain = E.ridge(Gp, dec, qp, 1.0, 0.0, 2, guard=False)
    if np.any(dec["lam"] == 0.0):                                   # the padding row of d = 63
        assert np.all(np.isnan(plain))
    else:
        res = float(np.linalg.norm(F.ridge_residual(m, q, 1.0, 0.0, plain[:d])))
        print(f"plain quotient: ||w|| {np.linalg.norm(plain):.3g}, residual / bound "
              f"{res / F.ridge_bound(m, q, 1.0, 0.0, 1e-13, 2, plain[:d]):.3g}")
    w = E.ridge(Gp, dec, qp, 1.0, 0.0, 2)
    assert np.all(np.isfinite(w)) and np.all(w[d:] == 0.0)
    res = float(np.linalg.norm(F.ridge_residual(m, q, 1.0, 0.0, w[:d])))
    assert res <= F.ridge_bound(m, q, 1.0, 0.0, 1e-13, 2, w[:d]), (case, res)
