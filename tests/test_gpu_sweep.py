"""The row-streaming passes (csrc/sweep_erm.hip: k_sweep_erm FUSED / VONLY / QONLY, k_sweep_erm_wide; csrc/sweep_multi.hip:
k_sweep_vm, k_sweep_qm) where a wave LOOPS, per kernel instance.

A wave (a workgroup of the wide kernel) takes the super-batches gw, gw + GW, ... of S*R rows; on the whole device one
round is 4096 to 65 536 rows, so in no other kernel-level test does a wave run its loop again while its results are
compared with a reference (test_gemv_linearity_large has 20 000 rows, on one f64 shape, and checks properties).  The
rbl_k_sweep_* entry points take the grid (num_cu) from the caller: with num_cu = 1 or 2 a wave is in its third super-batch after tens to a few hundred rows.
Every instance of tests/sweep_fixtures.TABLE runs at its narrowest and widest width and one with padded columns, at row
counts around one super-batch, around one round and in the third round with ragged ends, on
    dyadic inputs       (exact in any summation order): the outputs equal the reference bit for bit;
    real-valued inputs  : the outputs stay within the bounds sweep_fixtures propagates from the project's two constants.
Each case prints its largest error / bound per output (pytest -s) before it asserts."""
import numpy as np
import pytest

import sweep_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl._lib


@pytest.fixture(scope="module")
def cus(L):
    """the device's compute units: the largest num_cu the entry points take"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


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
        print(f"sweep-ratio {what} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(self.items())))


# ------------------------------------------------------------------------------------------------ the fused pass
def _fused_dyadic(L, cus, st, inst, d):
    fx = F.dyadic("fused", st, inst, d)
    sr = inst.r * inst.s
    for num_cu, counts in ((1, F.row_counts("fused", inst, 1)), (2, F.row_counts("fused", inst, 2)), (cus, [sr + 1])):
        for n in counts:
            ctx = (st, d, num_cu, n)
            args = (fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n], fx.sigma0, fx.rho, fx.rho_next, "hinge", st, num_cu)
            a = L.k_sweep_erm(*args, want_v=True)
            assert a["instance"] == F.reported("fused", inst, num_cu), ctx
            for name in ("lam", "v", "z"):
                assert np.array_equal(a[name], fx.ref[name][:n]), (name, ctx)
            assert np.array_equal(a["q"], fx.ref["q"][n]), ctx
            assert a["primal2"] == fx.ref["primal2"][n] and a["zz"] == fx.ref["zz"][n], ctx
            b = L.k_sweep_erm(*args, want_v=False)
            assert np.all(np.isnan(b["v"])), ctx                    # no store of v at all
            for name in ("lam", "z", "q", "primal2", "zz"):
                assert bits(a[name]) == bits(b[name]), (name, ctx)


def _fused_real(L, cus, st, inst, d, loss, rho, ratios):
    fx = F.real("fused", st, inst, d, loss, rho)
    sr = inst.r * inst.s

    def run(n, num_cu, want_v=True):
        out = L.k_sweep_erm(fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n], fx.sigma0, fx.rho, fx.rho_next, loss, st, num_cu, want_v)
        ctx = ("fused", loss, st, d, rho, num_cu, n)
        assert out["instance"] == F.reported("fused", inst, num_cu), ctx
        ref, err = fx.sums(n)
        for name in ("v", "lam", "z", "q", "primal2", "zz"):
            if name == "v" and not want_v:
                continue
            ratios.within(name, out[name], ref[name], err[name], ctx)
        return out

    one = {n: run(n, 1) for n in F.row_counts("fused", inst, 1)}
    both = {n: run(n, 2) for n in F.row_counts("fused", inst, 2)}
    for n in F.looping_rows("fused", inst, 2):
        two = both[n]
        base = one[n] if n in one else run(n, 1)
        for name in ("lam", "v", "z"):      # row-wise: the same bits on either grid; the sums change order with the grid
            assert bits(two[name]) == bits(base[name]), (name, loss, st, d, n)
    n = max(one)
    b = run(n, 1, want_v=False)
    assert np.all(np.isnan(b["v"]))
    for name in ("lam", "z", "q", "primal2", "zz"):
        assert bits(one[n][name]) == bits(b[name]), (name, loss, st, d)
    run(sr + 1, cus)                          # nearly every block idle: they must contribute zeros


@pytest.mark.parametrize("loss", F.LOSSES)
@pytest.mark.parametrize("case", F.cases("fused"), ids=F.case_id)
def test_fused_pass(L, cus, case, loss):
    st, inst = case
    ratios = Ratios()
    for i, d in enumerate(F.widths(st, inst)):
        if loss == "hinge":
            _fused_dyadic(L, cus, st, inst, d)
        _fused_real(L, cus, st, inst, d, loss, F.rho_of("fused", case, i), ratios)
    ratios.report(f"fused {loss} {F.case_id(case)}")


# ------------------------------------------------------------------------------------------------ V-only and Q-only
@pytest.mark.parametrize("case", F.cases("v"), ids=F.case_id)
def test_v_only_pass(L, cus, case):
    st, inst = case
    sr = inst.r * inst.s
    ratios = Ratios()
    for i, d in enumerate(F.widths(st, inst)):
        fx = F.dyadic("v", st, inst, d)
        for num_cu, counts in ((1, F.row_counts("v", inst, 1)), (2, F.row_counts("v", inst, 2)), (cus, [sr + 1])):
            for n in counts:
                ctx = ("v", st, d, num_cu, n)
                a = L.k_sweep_v(fx.D[:n], fx.w, fx.z_old[:n], fx.lam[:n], fx.rho, st, num_cu)
                assert a["instance"] == F.reported("v", inst, num_cu), ctx
                assert np.array_equal(a["v"], fx.ref["v"][:n]) and np.array_equal(a["lam"], fx.ref["lam"][:n]), ctx
                assert a["primal2"] == fx.ref["primal2"][n], ctx
        rho = F.rho_of("v", case, i)
        rx = F.real("v", st, inst, d, None, rho)

        def run(n, num_cu):
            out = L.k_sweep_v(rx.D[:n], rx.w, rx.z_old[:n], rx.lam[:n], rho, st, num_cu)
            ref, err = rx.sums(n)
            for name in ("v", "lam", "primal2"):
                ratios.within(name, out[name], ref[name], err[name], ("v", st, d, rho, num_cu, n))
            return out

        one = {n: run(n, 1) for n in F.row_counts("v", inst, 1)}
        both = {n: run(n, 2) for n in F.row_counts("v", inst, 2)}
        for n in F.looping_rows("v", inst, 2):
            two = both[n]
            base = one[n] if n in one else run(n, 1)
            assert bits(two["v"]) == bits(base["v"]) and bits(two["lam"]) == bits(base["lam"]), (st, d, n)
        run(sr + 1, cus)
    ratios.report(f"v {F.case_id(case)}")


@pytest.mark.parametrize("case", F.cases("q"), ids=F.case_id)
def test_q_only_pass(L, cus, case):
    st, inst = case
    sr = inst.r * inst.s
    ratios = Ratios()
    for d in F.widths(st, inst):
        fx = F.dyadic("q", st, inst, d)
        rx = F.real("q", st, inst, d, None, 1.0)
        for num_cu, counts in ((1, F.row_counts("q", inst, 1)), (2, F.row_counts("q", inst, 2)), (cus, [sr + 1])):
            for n in counts:
                ctx = ("q", st, d, num_cu, n)
                a = L.k_sweep_q(fx.D[:n], fx.c_in[:n], st, num_cu)
                assert a["instance"] == F.reported("q", inst, num_cu), ctx
                assert np.array_equal(a["q"], fx.ref["q_only"][n]), ctx
                q, e_q = rx.q_only(n)
                ratios.within("q", L.k_sweep_q(rx.D[:n], rx.c_in[:n], st, num_cu)["q"], q, e_q, ctx)
    ratios.report(f"q {F.case_id(case)}")


# ------------------------------------------------------------------------------------------------ the multi-column passes
@pytest.mark.parametrize("case", F.cases("multi_v"), ids=F.case_id)
def test_multi_v_pass(L, cus, case):
    """dyadic: k = 2 and k = 4 columns (the two column counts the kernels are compiled for) equal the reference in bits.
    Real-valued: column j of a k-column launch has the bits of the single-column pass on the same inputs and grid
    (header of sweep_multi.hip), k = 1..4, a rho per column, at the row counts where the waves loop.
    Slots >= k: the launcher hands the kernel column 0's pointers and rho for them, and the kernel skips their stores.  A
    store it did not skip would write column 0's own values onto column 0, so it cannot be told from outside; what is
    held here is that columns 0 .. k - 1 have the single-column pass' bits whatever k is.  The rows >= k of the arrays
    the entry point returns are buffers no launch is told about: their NaN only says that no column ran past its n
    rows into the next buffer."""
    st, inst = case
    sr = inst.r * inst.s
    for d in F.widths(st, inst):
        fx = F.dyadic("multi_v", st, inst, d)
        for num_cu, counts in ((1, F.row_counts("multi_v", inst, 1)), (2, F.row_counts("multi_v", inst, 2)), (cus, [sr + 1])):
            for n in counts:
                for k in (2, 4):
                    ctx = ("multi_v", st, d, num_cu, n, k)
                    a = L.k_sweep_v_multi(fx.D[:n], fx.W[:k], fx.Z[:k, :n], fx.LAM[:k, :n], fx.rho[:k], st, num_cu)
                    assert a["instance"] == F.reported("multi_v", inst, num_cu), ctx
                    assert np.array_equal(a["v"][:k], fx.ref["v"][:k, :n]), ctx
                    assert np.array_equal(a["lam"][:k], fx.ref["lam"][:k, :n]), ctx
                    assert [a["primal2"][j] for j in range(k)] == [fx.ref["primal2"][j][n] for j in range(k)], ctx
                    assert np.all(np.isnan(a["v"][k:])) and np.all(np.isnan(a["lam"][k:])), ctx   # (the entry's own buffers)
        D, W, Z, LAM, _ = F.real_multi("multi_v", st, inst, d)
        rho = np.array([2e-7, 1e-3, 1.0, 40.0])
        for num_cu in (1, 2):
            for n in F.looping_rows("multi_v", inst, num_cu):
                single = [L.k_sweep_v(D[:n], W[j], Z[j, :n], LAM[j, :n], rho[j], st, num_cu) for j in range(4)]
                for k in (1, 2, 3, 4):
                    ctx = ("multi_v real", st, d, num_cu, n, k)
                    a = L.k_sweep_v_multi(D[:n], W[:k], Z[:k, :n], LAM[:k, :n], rho[:k], st, num_cu)
                    for j in range(k):
                        assert bits(a["v"][j]) == bits(single[j]["v"]), (ctx, j)
                        assert bits(a["lam"][j]) == bits(single[j]["lam"]), (ctx, j)
                        assert bits(a["primal2"][j]) == bits(single[j]["primal2"]), (ctx, j)


@pytest.mark.parametrize("case", F.cases("multi_q"), ids=F.case_id)
def test_multi_q_pass(L, cus, case):
    st, inst = case
    sr = inst.r * inst.s
    for d in F.widths(st, inst):
        fx = F.dyadic("multi_q", st, inst, d)
        for num_cu, counts in ((1, F.row_counts("multi_q", inst, 1)), (2, F.row_counts("multi_q", inst, 2)), (cus, [sr + 1])):
            for n in counts:
                for k in (2, 4):
                    ctx = ("multi_q", st, d, num_cu, n, k)
                    a = L.k_sweep_q_multi(fx.D[:n], fx.C[:k, :n], st, num_cu)
                    assert a["instance"] == F.reported("multi_q", inst, num_cu), ctx
                    assert np.array_equal(a["q"], fx.ref["q"][n][:k]), ctx
        D, _, _, _, Cm = F.real_multi("multi_q", st, inst, d)
        for num_cu in (1, 2):
            for n in F.looping_rows("multi_q", inst, num_cu):
                single = [L.k_sweep_q(D[:n], Cm[j, :n], st, num_cu)["q"] for j in range(4)]
                for k in (1, 2, 3, 4):
                    a = L.k_sweep_q_multi(D[:n], Cm[:k, :n], st, num_cu)
                    for j in range(k):
                        assert bits(a["q"][j]) == bits(single[j]), ("multi_q real", st, d, num_cu, n, k, j)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(L, cus):
    """widths outside a pass' range and num_cu outside 1 .. the device's count are errors, checked before any launch"""
    rng = np.random.default_rng(0)

    def data(n, d, k=1):
        return rng.standard_normal((n, d)), rng.standard_normal((k, d)), rng.standard_normal((k, n))

    for st, d in (("f32", 128), ("f32", 16385), ("f64", 64), ("f64", 8193), ("fp16", 256), ("fp16", 16385)):
        D, w, z = data(8, d)
        assert F.lookup("fused", st, d) is None
        with pytest.raises(ValueError, match="outside the single-sweep"):
            L.k_sweep_erm(D, w[0], z[0], z[0], 0.01, 1.0, 1.02, "hinge", st, 1)
    for st, d in (("f32", 128), ("f32", 2049), ("f64", 1025), ("fp16", 256), ("fp16", 4097)):
        D, w, z = data(8, d)
        assert F.lookup("v", st, d) is None
        with pytest.raises(ValueError, match="outside the V-only"):
            L.k_sweep_v(D, w[0], z[0], z[0], 1.0, st, 1)
        with pytest.raises(ValueError, match="outside the Q-only"):
            L.k_sweep_q(D, z[0], st, 1)
    for st, d in (("f32", 2049), ("f64", 64), ("fp16", 2049)):
        D, w, z = data(8, d, 2)
        assert F.lookup("multi_v", st, d) is None
        with pytest.raises(ValueError, match="outside the multi-column"):
            L.k_sweep_v_multi(D, w, z, z, np.ones(2), st, 1)
        with pytest.raises(ValueError, match="outside the multi-column"):
            L.k_sweep_q_multi(D, z, st, 1)
    D, w, z = data(8, 300, 5)
    for num_cu in (0, -1, cus + 1):
        for call in (lambda: L.k_sweep_erm(D, w[0], z[0], z[0], 0.01, 1.0, 1.02, "hinge", "f32", num_cu),
                     lambda: L.k_sweep_v(D, w[0], z[0], z[0], 1.0, "f32", num_cu),
                     lambda: L.k_sweep_q(D, z[0], "f32", num_cu),
                     lambda: L.k_sweep_v_multi(D, w[:2], z[:2], z[:2], np.ones(2), "f32", num_cu),
                     lambda: L.k_sweep_q_multi(D, z[:2], "f32", num_cu)):
            with pytest.raises(ValueError, match="num_cu"):
                call()
    with pytest.raises(ValueError, match="columns"):
        L.k_sweep_v_multi(D, w, z, z, np.ones(5), "f32", 1)
    with pytest.raises(ValueError, match="columns"):
        L.k_sweep_q_multi(D, z, "f32", 1)
    with pytest.raises(ValueError, match="storage"):
        L.k_sweep_q(D, z[0], "csr", 1)
    assert L.k_sweep_q(D, z[0], "f32", cus)["instance"] == F.reported("q", F.lookup("q", "f32", 300), cus)
