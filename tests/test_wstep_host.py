"""The w-step fixtures (tests/wstep_fixtures.py) checked on the CPU before the GPU sees them: the instance table's
arithmetic, the planted minimisers' optimality in longdouble, the exactness of the integer fixtures, and a plain NumPy CG
at the kernels' stop rule held against the bounds the GPU tests use."""
import numpy as np
import pytest

import wstep_fixtures as F

LD = F.LD
HOST_D = [1, 3, 20, 252, 1028, 2052]


def test_instance_table_follows_from_the_constants():
    for ld in range(0, 2200, 4):
        assert F.instance(ld) == F.instance_from_constants(ld), ld
    # the ranges tile [4, WSTEP_PERSIST_MAX_LD] without gap or overlap, in multiples of 4
    assert F.INSTANCES[0][0] == 4 and F.INSTANCES[-1][1] == F.WSTEP_PERSIST_MAX_LD
    for a, b in zip(F.INSTANCES, F.INSTANCES[1:]):
        assert b[0] == a[1] + 4
    # the LDS boundary: rows of G and the fixed part fill the budget up to 1168, not at 1172
    assert F.instance(1168)["lds_bytes"] <= F.LDS_BUDGET < 8 * (1172 + 48) + 8 * 16 * 1172
    assert F.instance(1168)["lds_bytes"] == 136 * 1168 + 384 and F.instance(1172)["lds_bytes"] == 8 * (1172 + 48)
    # every width the GPU tests name is an edge of something: a slot boundary of 2 (k >> 1) 256 + ..., a block count, a range
    assert [F.instance(w)["per"] for w in (1024, 1028)] == [4, 8]
    assert [F.instance(w)["glds"] for w in (1168, 1172)] == [1, 0]
    assert [F.instance(w)["nblocks"] for w in (4, 16, 20, 2048)] == [1, 1, 2, 128]
    assert F.instance(2052) is None and F.instance(0) is None
    assert all(F.round_up(d, 4) in F.WIDTHS for d in F.PERSIST_D + F.BATCHED_ROUTE1_D + F.BATCHED_NATURAL_D if d != 4100)


@pytest.mark.parametrize("kind", ["well", "ill"])
def test_matrices_are_exact_and_inside_their_bounds(kind):
    for d in (3, 20, 252):
        m = F.matrix(d, kind)
        ev = np.linalg.eigvalsh(m.G)
        assert np.array_equal(m.G, m.G.T)
        slack = 1e-13 * m.lam_hi                                    # the eigensolver's own error, a few eps ||G||
        assert m.lam_lo - slack <= ev[0] and ev[-1] <= m.lam_hi + slack, (d, ev[0], ev[-1])
        assert (m.lam_lo >= 1.0) if kind == "well" else (m.lam_lo == 2.0 ** -20)
    mc, D = F.collinear(20)
    assert D.shape[0] > D.shape[1]
    assert np.array_equal(mc.G[:, 5], 2 * mc.G[:, 3] - mc.G[:, 4]) and np.array_equal(mc.G, D.T @ D)


def ulps_of_absGw(m, resid, w, extra=0.0):
    return float(np.max(np.abs(resid) / (F.absGw(m, w) + extra + 1e-300))) / F.EPS


@pytest.mark.parametrize("d", HOST_D)
def test_planted_minimisers_satisfy_their_optimality_conditions(d):
    """each w* against its own condition, in longdouble, to a few ulps of |G| |w*| (q was rounded once to fp64)"""
    for kind, rho, reg in (("well", 1.0, 0.5), ("well", 1e-3, 0.05), ("ill", 1.0, 2.0 ** -20)):
        m = F.matrix(d, kind)
        l2 = np.arange(d) % 5 + 1.0
        for pen in (None, l2):
            w, q = F.plant_ridge(m, rho, reg, pen)
            r = F.ridge_residual(m, q, rho, reg, w, pen) / LD(rho)
            assert ulps_of_absGw(m, r, w, np.abs(w) * (reg + 5.0) / rho) <= 2.0
        for t in (1.0, 1e-2):
            w, q = F.plant_huber(m, rho, reg, t)
            g = F.huber_gradient(m, q, rho, reg, t, w) / LD(rho)
            assert ulps_of_absGw(m, g, w, 0.5 * reg / rho) <= 2.0
            assert np.any(np.abs(w) < t) and (d == 1 or np.any(np.abs(w) > t))
            assert np.any(np.abs(np.abs(w) - t) <= 1e-3 * t)
    m = F.matrix(d, "well")
    for nnz in (1, 8, 64, 96, 97, 200):
        if nnz > d:
            continue
        for kappa in (0.75, 0.25 + (np.arange(d) % 4) / 4.0):
            w, q, s = F.plant_lasso(m, kappa, nnz)
            assert np.count_nonzero(w) == nnz and np.max(np.abs(s[w == 0]), initial=0.0) <= 0.9
            kap = np.broadcast_to(kappa, (d,))
            # on the support the condition holds to rounding; off it with the slack the fixture planted
            g = m.mv(w) - q.astype(LD)
            on = w != 0
            assert ulps_of_absGw(m, np.where(on, g + kap * np.sign(w), 0), w, kap) <= 2.0
            assert np.all(np.abs(g[~on]) <= 0.9 * kap[~on] + 2 * F.EPS * (F.absGw(m, w) + kap)[~on])
            assert F.lasso_kkt(m, q, kappa, w) <= 2 * F.EPS * float(np.max(F.absGw(m, w) + kap))


@pytest.mark.parametrize("d", [1, 3, 20, 516, 2048])
def test_integer_fixtures_are_exact(d):
    G, w0, p = F.integer_fixture(d)
    assert np.unique(G % p).size == d * d                          # all entries different modulo the prime
    assert np.all(np.abs(w0) >= 1) and np.all(np.abs(w0) <= 3)
    for l2 in (False, True):
        Gf, wf, q, Gw, pen = F.integer_ridge(d, l2)
        assert np.array_equal(Gf.astype(np.int64), G) and np.array_equal(q.astype(np.int64), Gw + (pen if l2 else 1) * w0)
        # the first residual of the CG, in the kernel's float64 and in any order: exactly zero
        assert np.array_equal((Gf @ wf) + (pen if l2 else 1.0) * wf, q)
        assert np.array_equal((Gf[:, ::-1] @ wf[::-1]), Gw.astype(np.float64))
    Gf, wf, q, Gw = F.integer_huber(d)
    assert np.array_equal((Gf @ wf - q) + F.hub_g(wf, 1.0, 0.5), np.zeros(d))


@pytest.mark.parametrize("d", HOST_D)
def test_numpy_cg_stays_within_the_bounds(d):
    """The restatement (not the code under test) at the kernels' stop rule.  Its true residual is inside the whole bound;
    the bound's first term is the stop rule itself (the recurrence residual ends at 0.3 - 1 times it, so no margin can be
    asked of it), the second models the drift between the true and the recurrence residual - that part keeps a margin
    of 4 or more.  The error in w is the residual over lambda_min(A) and inherits the residual's bound as it is."""
    tol = 1e-13
    for kind, rho, reg in (("well", 1.0, 0.5), ("well", 1e-3, 0.05), ("ill", 1.0, 2.0 ** -20)):
        m = F.matrix(d, kind)
        for pen in (None, np.arange(d) % 5 + 1.0):
            ws, q = F.plant_ridge(m, rho, reg, pen)
            w_cold, it_cold, _ = F.cg_numpy(m.G, q, rho, reg, tol, np.zeros(d), pen)
            q2 = q + 1e-4 * np.max(np.abs(q)) * np.random.default_rng(d).standard_normal(d)
            for start, rhs in ((np.zeros(d), q), (w_cold, q2)):
                w, it, rk = F.cg_numpy(m.G, rhs, rho, reg, tol, start, pen)
                assert it < 4000                                    # the persistent kernel's cap
                if kind == "ill" and d >= 252 and pen is None and start is not w_cold:
                    assert it >= 100, it                            # "hundreds of iterations"
                true = -F.ridge_residual(m, rhs, rho, reg, w, pen)
                res = float(np.linalg.norm(true))
                assert res <= F.ridge_bound(m, rhs, rho, reg, tol, it, w, pen), (kind, d, it)
                drift = float(np.linalg.norm(true - rk.astype(LD)))
                allowed = it * 4 * F.EPS * F.a_hi(m, rho, reg, pen) * float(np.linalg.norm(w))
                assert 4 * drift <= allowed, (kind, d, it, drift / allowed)
                if rhs is q:
                    err = float(np.linalg.norm(w - ws))
                    assert err <= F.ridge_w_bound(m, q, rho, reg, tol, it, w, pen), (kind, d, it)


def test_sequence_fixture_makes_the_jumps_cost_a_second_batch():
    """the drifting right-hand sides: by the restatement, a jump step needs more CG iterations than the step before it
    plus 2 (the batch the batched route enqueues), with room for the device's count to differ by one"""
    for d in F.SEQ_D:
        m = F.matrix(d, "well")
        _, q0 = F.plant_ridge(m, F.SEQ_RHO, F.SEQ_REG)
        Q = F.drifting_rhs(q0)
        w, its = np.zeros(d), []
        for k in range(Q.shape[0]):
            w, it, _ = F.cg_numpy(m.G, Q[k], F.SEQ_RHO, F.SEQ_REG, 1e-13, w)
            its.append(it)
        for k in F.SEQ_JUMPS:
            assert its[k] >= its[k - 1] + 2 + 2, (d, its)
