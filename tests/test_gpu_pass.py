"""The plain passes (csrc/sweep.hip: k_gemv, k_gemvt, its column-statistics variant SQ, k_colreduce) and the Gram kernels
(csrc/gram.hip: k_gram, k_gram_reduce), per kernel instance, where a wave or a block LOOPS.

The rbl_k_pass_* / rbl_k_gram_full entry points take the grid (num_cu) from the caller and return what the launchers
picked; with num_cu = 1 or 2 a k_gemv wave is in its third round and a k_gemvt block in its third step after tens to a
few thousand rows.  Every instance of the tables of tests/pass_fixtures runs at its narrowest and widest width and one
with padded columns, at row counts around one step, around one round and in the third with ragged ends, on
    dyadic inputs       (exact in any summation order): the outputs equal the integer reference bit for bit;
    real-valued inputs  : the outputs stay within the bounds pass_fixtures states from the project's constant.
Outputs over the columns come back at their full length ld: the pad is +0.0 bit for bit, as the w-step and eig.hip need.
Each case prints its largest error / bound per output (pytest -s) before it asserts."""
import numpy as np
import pytest

import pass_fixtures as F
import sweep_fixtures as S
from test_gpu_sweep import L, Ratios, bits, cus   # noqa: F401  (L and cus are fixtures)

pytestmark = pytest.mark.gpu


class PassRatios(Ratios):
    def report(self, what):
        print(f"pass-ratio {what} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(self.items())))


def pad_is_plus_zero(x, d):
    return bits(x[d:]) == bytes(8 * (len(x) - d))


def exact(got, ref):
    """the reference's bits (the sums are non-zero or +0.0 in the reference, so array_equal would let a -0.0 through)"""
    return bits(got) == bits(np.asarray(ref, dtype=np.float64) + 0.0)


# ------------------------------------------------------------------------------------------------ v = D w
@pytest.mark.parametrize("case", F.cases("v"), ids=F.case_id)
def test_v_pass(L, cus, case):
    st, inst = case
    rs = (64 // inst.lpr) * inst.u
    ratios = PassRatios()
    for d in F.widths(st, inst):
        fx, rx = F.dyadic_v(st, inst, d), F.real_v(st, inst, d)
        for num_cu, counts in ((1, F.gemv_row_counts(inst, 1)), (2, F.gemv_row_counts(inst, 2)), (cus, [rs + 1])):
            for n in counts:
                ctx = ("v", st, d, num_cu, n)
                a = L.k_pass_v(fx.D[:n], fx.w, st, num_cu)
                assert a["instance"] == F.gemv_reported(inst, num_cu, n), ctx
                assert not np.any(np.isnan(a["v"])), (ctx, "a row was not written")
                assert np.array_equal(a["v"], fx.ref["v"][:n]), ctx
                b = L.k_pass_v(rx.D[:n], rx.w, st, num_cu)
                ratios.within("v", b["v"], rx.v[:n], rx.e_v[:n], ctx)
    ratios.report(f"v {F.case_id(case)}")


@pytest.mark.parametrize("st", S.STORAGES)
def test_v_pass_refuses_rows_wider_than_the_lds(L, st):
    """150 KiB of w do not fit the LDS-staged path: RBL_ERR_INVALID before anything is launched"""
    d = F.refused_width(st)
    assert F.lookup("v", st, d) is None and F.lookup("v", st, d - 1) is not None
    D = np.ones((2, d))
    with pytest.raises(ValueError, match="too large for the LDS-staged path"):
        L.k_pass_v(D, np.ones(d), st, 1)
    assert L.k_pass_v(D[:, :d - 1], np.ones(d - 1), st, 1)["v"].tolist() == [d - 1.0, d - 1.0]


# ------------------------------------------------------------------------------------------------ q = D^T c
@pytest.mark.parametrize("case", F.cases("q"), ids=F.case_id)
def test_q_pass(L, cus, case):
    st, inst = case
    s = (256 // inst.tpr) * inst.u
    ratios = PassRatios()
    for d in F.widths(st, inst):
        fx, rx = F.dyadic_q(st, inst, d), F.real_q(st, inst, d)
        for num_cu, n in F.gemvt_grids(inst) + [(cus, s + 1)]:
            ctx = ("q", st, d, num_cu, n)
            a = L.k_pass_q(fx.D[:n], fx.c[:n], st, num_cu)
            assert a["instance"] == F.gemvt_reported(inst, num_cu, n), ctx
            assert exact(a["q"][:d], fx.ref["q"][n]) and pad_is_plus_zero(a["q"], d), ctx
            b = L.k_pass_q(rx.D[:n], rx.c[:n], st, num_cu)
            ratios.within("q", b["q"][:d], rx.q[n], rx.e_q[n], ctx)
            assert pad_is_plus_zero(b["q"], d), ctx
    ratios.report(f"q {F.case_id(case)}")


@pytest.mark.parametrize("st", S.STORAGES)
def test_q_pass_hands_33_to_512_packets_to_the_q_only_pass(L, st):
    """launch_gemvt routes these widths to launch_sweep_q (tests/test_gpu_sweep.py holds those kernels to their
    reference): only the reported instance is asserted here, at both ends of the range"""
    rng = np.random.default_rng(5)
    for d in (32 * S.PACKET[st] + 1, 512 * S.PACKET[st]):
        inst = S.lookup("q", st, d)
        assert inst is not None and F.lookup("q", st, d) is None
        for num_cu in (1, 2):
            a = L.k_pass_q(rng.standard_normal((40, d)), rng.standard_normal(40), st, num_cu)
            assert a["instance"] == ("sweep_q",) + S.reported("q", inst, num_cu)[1:], (st, d, num_cu)
            assert pad_is_plus_zero(a["q"], d)


def test_q_pass_blocks_without_rows(L, cus):
    """the whole device at the narrowest instance, n from the CU count: nb is capped at 4 x CUs and the last block's
    range starts at row n - it must add zeros to every column"""
    n = F.empty_tail_rows(cus)
    assert n is not None, "the device is too small for a capped grid with an empty block"
    nb = 4 * cus
    assert F.gemvt_nb(cus, n) == nb and (nb - 1) * F.gemvt_rows_per_block(cus, n) >= n
    for st in S.STORAGES:
        d = 3
        inst = F.lookup("q", st, d)
        fx = F.DyadicPass(st, d, n, [n], (), S.seed_of("empty_tail", st))
        assert fx.exactness_report() == []
        a = L.k_pass_q(fx.D, fx.c, st, cus)
        assert a["instance"] == F.gemvt_reported(inst, cus, n) and a["instance"][3] == nb
        assert exact(a["q"][:d], fx.ref["q"][n]) and pad_is_plus_zero(a["q"], d), st
        if st in F.COLSTATS_STORAGES:
            b = L.k_pass_colstats(fx.D, st, cus)
            assert exact(b["sum"][:d], fx.ref["sum"][n]) and exact(b["sumsq"][:d], fx.ref["sumsq"][n]), st


# ------------------------------------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("case", F.cases("colstats"), ids=F.case_id)
def test_colstats_pass(L, cus, case):
    st, inst = case
    s = (256 // inst.tpr) * inst.u
    ratios = PassRatios()
    for d in F.widths(st, inst):
        fx, rx = F.dyadic_q(st, inst, d), F.real_q(st, inst, d)
        for num_cu, n in F.gemvt_grids(inst) + [(cus, s + 1)]:
            ctx = ("colstats", st, d, num_cu, n)
            a = L.k_pass_colstats(fx.D[:n], st, num_cu)
            assert a["instance"] == F.gemvt_reported(inst, num_cu, n), ctx
            assert exact(a["sum"][:d], fx.ref["sum"][n]) and exact(a["sumsq"][:d], fx.ref["sumsq"][n]), ctx
            assert pad_is_plus_zero(a["sum"], d) and pad_is_plus_zero(a["sumsq"], d), ctx
            b = L.k_pass_colstats(rx.D[:n], st, num_cu)
            ratios.within("sum", b["sum"][:d], rx.sum[n], rx.e_sum[n], ctx)
            ratios.within("sumsq", b["sumsq"][:d], rx.sumsq[n], rx.e_sumsq[n], ctx)
            assert pad_is_plus_zero(b["sum"], d) and pad_is_plus_zero(b["sumsq"], d), ctx
    ratios.report(f"colstats {F.case_id(case)}")


def test_colstats_pass_refuses_fp16(L):
    with pytest.raises(ValueError, match="not available for RBL_STORE_F16"):
        L.k_pass_colstats(np.ones((4, 4)), "fp16", 1)


# ------------------------------------------------------------------------------------------------ G = D^T D
@pytest.mark.parametrize("case", F.gram_cases(), ids=lambda c: f"{c[0]}-d{c[1]}")
def test_gram(L, cus, case):
    st, d = case
    ld = S.ld_of(d, st)
    fx, rx = F.dyadic_gram(st, d), F.real_gram(st, d)
    ratios = PassRatios()

    def run(D, n, num_cu):
        ctx = ("gram", st, d, num_cu, n)
        a = L.k_gram_full(D[:n], st, num_cu)
        G = a["G"]
        assert a["plan"] == F.gram_plan(ld, n, num_cu), ctx
        assert np.all(np.isfinite(G)), (ctx, "an entry was left at 0xff")
        assert bits(G) == bits(G.T), ctx
        pad = np.ones((ld, ld), dtype=bool)
        pad[:d, :d] = False
        assert bits(G[pad]) == bytes(8 * int(pad.sum())), (ctx, "pad rows and columns must be +0.0")
        assert bits(L.k_gram_full(D[:n], st, num_cu)["G"]) == bits(G), (ctx, "a second call returns the same bits")
        return G[:d, :d]

    for num_cu in (1, 2, cus):
        for n in F.GRAM_ROWS:
            assert exact(run(fx.D, n, num_cu), fx.ref[n]), ("gram", st, d, num_cu, n)
        for n in F.GRAM_REAL_ROWS:
            G = run(rx.D, n, num_cu)
            err = np.abs(G - rx.G[n])
            r = float(np.max(err / rx.scale[n]))
            ratios["G/DOT"] = max(ratios.get("G/DOT", 0.0), r)          # printed, not asserted: nobody has measured it
            ratios["G/1e-12n"] = max(ratios.get("G/1e-12n", 0.0), float(np.max(err)) / (1e-12 * n))
            if float(np.max(err)) > 1e-12 * n:
                ratios.report(f"gram {st} d={d}")
            assert float(np.max(err)) <= 1e-12 * n, ("gram", st, d, num_cu, n)
    ratios.report(f"gram {st} d={d}")


# ------------------------------------------------------------------------------------------------ refusals
def test_pass_refusals(L, cus):
    """num_cu outside 1 .. the device's count, empty inputs and sparse storage are errors, checked before any launch"""
    D, w, c = np.ones((8, 12)), np.ones(12), np.ones(8)
    for num_cu in (0, -1, cus + 1):
        for call in (lambda: L.k_pass_v(D, w, "f32", num_cu), lambda: L.k_pass_q(D, c, "f32", num_cu),
                     lambda: L.k_pass_colstats(D, "f32", num_cu), lambda: L.k_gram_full(D, "f32", num_cu)):
            with pytest.raises(ValueError, match="num_cu"):
                call()
    for call in (lambda: L.k_pass_v(D, w, "csr", 1), lambda: L.k_pass_q(D, c, "csr", 1),
                 lambda: L.k_pass_colstats(D, "csr", 1), lambda: L.k_gram_full(D, "csr", 1)):
        with pytest.raises(ValueError, match="storage"):
            call()
    assert L.k_pass_v(D, w, "f32", cus)["instance"] == F.gemv_reported(F.lookup("v", "f32", 12), cus, 8)
