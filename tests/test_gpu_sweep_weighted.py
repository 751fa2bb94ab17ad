"""The row-weighted twins of the single-sweep erm kernels (csrc/sweep_erm.hip: SE_FUSED_W of k_sweep_erm, WT of
k_sweep_erm_wide; compiled in csrc/sweep_erm_w.hip) through rbl_k_sweep_erm_w: one sigma per row in the place of sigma0.

Every fused instance of tests/sweep_fixtures.TABLE runs at its narrowest and widest width and one with padded columns,
with num_cu 1 and 2, at the row counts of sweep_fixtures.row_counts (a wave or workgroup loops: the third round has a
ragged last super-batch and sub-batch); the reported instance must be the table's.
    identity     sigma_i = sigma0 for all i: every output has the bits of rbl_k_sweep_erm on the same inputs (all losses);
    placement    dyadic inputs, hinge, c_i from {0, 1/4, 1/2, 1, 2, 4} with no row carrying the weight of a neighbour or of
                 the row S*R or GW*S*R before it, zeros on row 0, row n - 1 and the last row of a full super-batch: the
                 device returns the integer reference's bits, and the reference itself changes when the weights are
                 taken from any of those other rows; where c_i = 0, z_new_i = v_i - lam_out_i / rho_next in bits;
    real-valued  c log-uniform on [1e-3, 1e3] with 10 % zeros, rho in {2e-7, 1e-3, 1}: the bounds of sweep_fixtures.Real,
                 unchanged (the prox is 1-Lipschitz in m whatever sigma is: no new constant); row-wise outputs have the
                 same bits on either grid; want_v = 0 gives the bits of want_v = 1.
Each case prints its largest error / bound per output (pytest -s) before it asserts."""
import numpy as np
import pytest

import sweep_fixtures as F

pytestmark = pytest.mark.gpu

WEIGHTS = (0.25, 0.5, 1.0, 2.0, 4.0)          # with 0.0: the family of the placement test


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl._lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


class Ratios(dict):
    """largest error / bound per output of one test"""

    def within(self, name, got, ref, err, ctx):
        got, ref, err = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(err, dtype=np.float64)
        assert np.all(np.isfinite(got)), (name, ctx, "a row was not written")
        r = float(np.max(np.abs(got - ref) / err))
        self[name] = max(self.get(name, 0.0), r)
        if r > 1.0:
            self.report(ctx)
        assert r <= 1.0, (name, ctx, r)

    def report(self, what):
        print(f"sweep-w-ratio {what} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(self.items())))


def zero_rows_are_m(out, c, rho_next, ctx):
    """c_i = 0: the prox is the identity, z_new_i has the bits of v_i - lam_out_i / rho_next from the device's own v, lam"""
    zero = np.flatnonzero(np.asarray(c) == 0.0)
    m = out["v"][zero] - out["lam"][zero] / rho_next
    assert bits(out["z"][zero]) == bits(m), ctx


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("case", F.cases("fused"), ids=F.case_id)
def test_constant_sigma_is_the_unweighted_pass(L, case):
    st, inst = case
    for i, d in enumerate(F.widths(st, inst)):
        for loss in F.LOSSES:
            fx = F.real("fused", st, inst, d, loss, F.rho_of("fused", case, i))
            for num_cu in (1, 2):
                for n in F.row_counts("fused", inst, num_cu):
                    ctx = (loss, st, d, num_cu, n)
                    args = (fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n])
                    tail = (fx.rho, fx.rho_next, loss, st, num_cu)
                    a = L.k_sweep_erm(*args, fx.sigma0, *tail)
                    b = L.k_sweep_erm_w(*args, np.full(n, fx.sigma0), *tail)
                    assert b["instance"] == a["instance"] == F.reported("fused", inst, num_cu), ctx
                    for name in ("lam", "v", "z", "q", "primal2", "zz"):
                        assert bits(a[name]) == bits(b[name]), (name, ctx)


# ------------------------------------------------------------------------------------------------ placement
def placement_weights(n, sr, gws):
    """c (n values of {0} + WEIGHTS): a row's weight differs from its neighbours' and from the rows sr and gw * sr (every
    gw of gws) before it; then zeros on row 0, row n - 1 and the last row of the first full super-batch"""
    shifts = sorted({1, sr} | {gw * sr for gw in gws})
    c = np.zeros(n)
    for i in range(n):
        taken = {c[i - k] for k in shifts if i - k >= 0}
        c[i] = next(x for x in WEIGHTS[i % 5:] + WEIGHTS[:i % 5] if x not in taken)
    zeros = {0, n - 1} | ({sr - 1} if n >= sr else set())
    for i in range(n):          # the non-zero rows keep the property; the prescribed zeros may meet each other (n = sr + 1)
        for k in shifts:
            if i - k >= 0 and i not in zeros and i - k not in zeros:
                assert c[i] != c[i - k], (n, i, k)
    c[sorted(zeros)] = 0.0
    return c, shifts


def weighted_hinge_units(fx, c, n):
    """the integer reference of sweep_fixtures.Dyadic with sigma_i = c_i * sigma0: (z', coefficient) in units of 2^-24"""
    lam1, v = fx.i_lam1[:n], fx.i_v[:n]
    lr = F._scale(lam1, 1.0 / fx.rho_next)
    m = v - lr
    s = F._to_units(c * fx.sigma0 / fx.rho_next)
    a = m - s
    zn = np.where(a >= -F.UNIT, a, np.where(m <= -F.UNIT, m, -F.UNIT))
    return zn, zn + lr


def q_units(fx, coef, n):
    """q = D^T coef exactly (sweep_fixtures.Dyadic._sums), asserting that any order of summation is exact"""
    t = F._trailing(coef)
    cc = coef >> t
    assert F.any_order_exact(int(np.max(np.abs(fx.D8[:n]).T @ np.abs(cc))), [1])
    return (fx.D8[:n].T @ cc).astype(np.float64) * (2.0 ** (t - F.UNIT_LOG - 3))


@pytest.mark.parametrize("case", F.cases("fused"), ids=F.case_id)
def test_weights_reach_their_own_rows(L, case):
    st, inst = case
    sr = inst.r * inst.s
    gws = [F.workers("fused", inst, k) for k in (1, 2)]
    for d in F.widths(st, inst):
        fx = F.dyadic("fused", st, inst, d)
        for num_cu in (1, 2):
            for n in F.row_counts("fused", inst, num_cu):
                ctx = (st, d, num_cu, n)
                c, shifts = placement_weights(n, sr, gws)
                zn, coef = weighted_hinge_units(fx, c, n)
                ref_z, ref_q = F._from_units(zn), q_units(fx, coef, n)
                ref_zz = F._sq_prefix(zn, [n])[n]
                if n > 2 * sr:    # the reference is sensitive: weights taken from another row give another z' and q
                    for k in [k for k in shifts if k < n] + [-1]:
                        zk, ck = weighted_hinge_units(fx, np.roll(c, k), n)
                        assert not np.array_equal(zk, zn) and not np.array_equal(q_units(fx, ck, n), ref_q), (ctx, k)
                sigma = c * fx.sigma0
                a = L.k_sweep_erm_w(fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n], sigma, fx.rho, fx.rho_next, "hinge", st, num_cu)
                assert a["instance"] == F.reported("fused", inst, num_cu), ctx
                assert np.array_equal(a["lam"], fx.ref["lam"][:n]) and np.array_equal(a["v"], fx.ref["v"][:n]), ctx
                bad = np.flatnonzero(a["z"] != ref_z)
                assert bad.size == 0, (ctx, "rows with another weight's z'", bad[:8].tolist(), c[bad[:8]].tolist())
                assert np.array_equal(a["q"], ref_q), ctx
                assert a["primal2"] == fx.ref["primal2"][n] and a["zz"] == ref_zz, ctx
                zero_rows_are_m(a, c, fx.rho_next, ctx)


# ------------------------------------------------------------------------------------------------ real-valued
def real_weights(n, seed):
    rng = np.random.default_rng(seed)
    c = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=n))
    c[rng.random(n) < 0.10] = 0.0
    c[0] = 0.0
    return c


def weighted_real(st, inst, d, loss, rho):
    """sweep_fixtures.Real with z' = prox(sigma_i, rho_next, m): the bounds are its own, unchanged"""
    fx = F.real("fused", st, inst, d, loss, rho)
    c = real_weights(fx.n, F.seed_of("w", st, d, loss))
    lr = fx.ref["lr"]
    m = fx.ref["v"] - lr
    z = F.prox(loss, c * fx.sigma0, fx.rho_next, m)
    fx.ref.update(z=z, c=z + lr)
    return fx, c


@pytest.mark.parametrize("loss", F.LOSSES)
@pytest.mark.parametrize("case", F.cases("fused"), ids=F.case_id)
def test_real_valued_weights(L, case, loss):
    st, inst = case
    ratios = Ratios()
    for i, d in enumerate(F.widths(st, inst)):
        rho = F.rho_of("fused", case, i)
        fx, c = weighted_real(st, inst, d, loss, rho)

        def run(n, num_cu, want_v=True):
            out = L.k_sweep_erm_w(fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n], c[:n] * fx.sigma0, fx.rho, fx.rho_next, loss, st,
                                  num_cu, want_v)
            ctx = ("fused_w", loss, st, d, rho, num_cu, n)
            assert out["instance"] == F.reported("fused", inst, num_cu), ctx
            ref, err = fx.sums(n)
            for name in ("v", "lam", "z", "q", "primal2", "zz"):
                if name == "v" and not want_v:
                    continue
                ratios.within(name, out[name], ref[name], err[name], ctx)
            if want_v:
                zero_rows_are_m(out, c[:n], fx.rho_next, ctx)
            return out

        one = {n: run(n, 1) for n in F.row_counts("fused", inst, 1)}
        both = {n: run(n, 2) for n in F.row_counts("fused", inst, 2)}
        for n in F.looping_rows("fused", inst, 2):
            base = one[n] if n in one else run(n, 1)
            for name in ("lam", "v", "z"):      # row-wise: the same bits on either grid
                assert bits(both[n][name]) == bits(base[name]), (name, loss, st, d, n)
        n = max(one)
        b = run(n, 1, want_v=False)
        assert np.all(np.isnan(b["v"]))
        for name in ("lam", "z", "q", "primal2", "zz"):
            assert bits(one[n][name]) == bits(b[name]), (name, loss, st, d)
    ratios.report(f"fused_w {loss} {F.case_id(case)}")
