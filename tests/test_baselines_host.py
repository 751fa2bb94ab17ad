"""What the kernel-level GPU tests of the competitor baselines (test_gpu_baselines_kernels.py) claim about their
inputs, pinned on a CPU: every exact fixture of tests/baseline_fixtures.py is certified against the restatement in
fractions.Fraction (the float64 oracle rounds nowhere, in any summation order) and has the features planted in it,
every smooth fixture moves w, and the case tables cover the trip counts and tails of csrc/baselines.hip."""
import numpy as np
import pytest

import baseline_fixtures as F

EXACT_SGD = [c for c in F.SGD_CASES if c.kind == "exact"]
EXACT_LSVRG = [c for c in F.LSVRG_CASES if c.kind == "exact"]
SMOOTH = [c for c in F.SGD_CASES + F.LSVRG_CASES if c.kind == "smooth"]
# the wrong answers (run_exact: mut) are run where an epoch in Fractions costs little
CHEAP_SGD = [c for c in EXACT_SGD if c.d * c.batch <= 5000]
CHEAP_LSVRG = [c for c in EXACT_LSVRG if c.d <= 63 and 2 <= c.n <= 257]
ids = lambda cases: [c.id for c in cases]


def _certify(P, ops):
    """oracle == Fraction restatement after every op; -> (exact ws, stats)"""
    ref = F.run_oracle(P, ops)
    ex, st = F.run_exact(P, ops)
    assert len(ref) == len(ex) == len(ops)
    for k, (a, b) in enumerate(zip(ref, ex)):
        assert F.equals_exact(a, b), f"op {k}: the float64 oracle rounds"
    assert 0 < st["bits"] < 53, st                       # every partial sum of every sum, in any order, is a float64
    return ex, st


def _differs(P, ops, ex, mut):
    return F.run_exact(P, ops, mut=mut)[0][-1] != ex[-1]


@pytest.mark.parametrize("case", EXACT_SGD, ids=ids(EXACT_SGD))
def test_exact_sgd_fixture_is_exact_and_has_its_features(case):
    P, ops = F.sgd_problem(case)
    n, order = P.X.shape[0], ops[1].order
    assert n & (n - 1) == 0 and n >= case.steps * case.batch + 5 and n // 2 < case.steps * case.batch + 5
    assert order.size == case.steps * case.batch == np.unique(order).size < n and np.any(np.diff(order) < 0)
    assert np.all(np.abs(P.X) <= 3) and np.all(P.X == np.round(P.X)) and set(np.unique(P.y01)) <= {0.0, 1.0}
    for w in (ops[1].ab, ops[1].bb):
        assert w is None or (w.size == case.batch and np.all(np.diff(w) > 0) and np.all(w * 2.0 ** 20 == np.round(w * 2.0 ** 20)))
    ex, st = _certify(P, ops)
    assert st["t0"] >= 1                                 # a row with y = 1 on the hinge tie at step 0
    if case.batch >= 2:
        assert st["ties"] >= 1
    if case.weights == "ehrm":
        assert case.d >= 2 and case.batch >= 2 and st["onB"] >= 1 and (st["sides"] == 3 or case.batch < 5)
    if case.reg == "l1":
        assert st["zeros"] >= 1 and set(ops[1].rands.tolist()) <= {0.25, 0.75}
    if case in CHEAP_SGD:
        assert _differs(P, ops, ex, "kink")
        assert _differs(P, ops, ex, "ties") or case.batch == 1


@pytest.mark.parametrize("case", EXACT_LSVRG, ids=ids(EXACT_LSVRG))
def test_exact_lsvrg_fixture_is_exact_and_has_its_features(case):
    P, ops = F.lsvrg_problem(case)
    assert P.X.shape == (case.n, case.d) and len(ops) == 1 + len(case.steps)
    a = ops[1].alphas
    assert a.size == case.n and np.all(np.diff(a) > 0) and (ops[1].betas is None) == (case.weights != "ehrm")
    if case.samples == "repeat":
        s = ops[1].samples
        assert s[1] == s[2] == s[3]
    ex, st = _certify(P, ops)
    assert st["t0"] >= 1
    if case.n >= 2:
        assert st["ties"] >= 1
    if case.weights == "ehrm" and case.n >= 5:
        assert st["onB"] >= 1 and st["sides"] == 3
    if case.reg == "l1":
        assert st["zeros"] >= 1
    if max(case.steps) >= 100 and case.n >= 2:
        assert st["ndiff"] >= 1                          # a step whose two derivatives differ: the variance term is live
    for k, steps in enumerate(case.steps):
        if steps == 0:
            assert ex[k + 1] == ex[k]                    # the checkpoint alone leaves w where it was
    if case in CHEAP_LSVRG:
        assert _differs(P, ops, ex, "kink") and _differs(P, ops, ex, "ties")


def test_uniform_sampling_by_row_index_is_visible():
    """alphas[row index] against alphas[row at that rank]: the exact uniform fixtures with 100 steps tell them apart"""
    cases = [c for c in EXACT_LSVRG if c.uniform and max(c.steps) >= 100 and c.d <= 255]
    assert len(cases) >= 2
    for case in cases:
        P, ops = F.lsvrg_problem(case)
        assert _differs(P, ops, F.run_exact(P, ops)[0], "uniform"), case.id


def test_exact_handle_sequence():
    P, ops = F.sequence_problem()
    kinds = [type(op).__name__ for op in ops]
    assert kinds == ["SetW", "Sgd", "Sgd", "Lsvrg", "SetW", "Sgd"]
    assert ops[1].steps * ops[1].batch < ops[2].steps * ops[2].batch and len(ops[3].samples) == 100 and P.l1 != 0
    ex, st = _certify(P, ops)
    assert st["zeros"] >= 1 and st["ties"] >= 1 and st["ndiff"] >= 1
    assert all(ex[k] != ex[k - 1] for k in range(1, len(ops)))


@pytest.mark.parametrize("case", SMOOTH, ids=ids(SMOOTH))
def test_smooth_fixture_moves(case):
    P, ops = (F.sgd_problem if isinstance(case, F.SgdCase) else F.lsvrg_problem)(case)
    assert P.loss == F.BCE and np.all(P.X * 256.0 == np.round(P.X * 256.0)) and set(np.unique(P.y01)) <= {0.0, 1.0}
    ws = F.run_oracle(P, ops)
    assert all(np.all(np.isfinite(w)) for w in ws)
    assert np.max(np.abs(ws[-1] - ws[0])) > 1e-3
    if case.reg == "l1":
        assert np.count_nonzero(P.w0 == 0.0) >= 1
    assert F.near_ties(P, ops) == 0                      # the order of the losses is the same to every libm


def test_the_tables_cover_the_edges():
    for kind in ("exact", "smooth"):
        sgd = [c for c in F.SGD_CASES if c.kind == kind]
        assert {c.batch % 4 for c in sgd} == {0, 1, 2, 3}                    # the logit phase's 4 rows per wave
        assert {c.batch % 8 for c in sgd} == (set(range(8)) if kind == "exact" else {0, 1, 2, 3, 5, 7})     # the 8-row tail
        assert {c.reg for c in sgd} == {"none", "l2", "l1"} and {c.weights for c in sgd} == {"inc", "ehrm"}
        assert {63, 64, 65, 1023, 1024, 1025} <= {c.d for c in sgd}          # a d on each side of a trip count
        lsv = [c for c in F.LSVRG_CASES if c.kind == kind]
        assert {255, 256, 257} <= {c.d for c in lsv} and min(c.d for c in lsv) < 64 and max(c.d for c in lsv) > 1024
        assert {c.uniform for c in lsv} == {0, 1} and {c.reg for c in lsv} == {"none", "l2", "l1"}
        assert {"repeat"} <= {c.samples for c in lsv} and {c.weights for c in lsv} == {"inc", "ehrm"}
    exact = [c for c in F.SGD_CASES if c.kind == "exact"]
    assert {c.d for c in exact} == set(F.SGD_D) == {c.d for c in F.SGD_CASES}
    assert {c.batch for c in exact} == set(F.SGD_BATCH) == {c.batch for c in F.SGD_CASES}
    assert {1, 2, 3, 1024} <= set(F.SGD_BATCH) and all(3 <= c.steps <= 5 for c in F.SGD_CASES)
    for d in (d for d in F.SGD_D if d >= 1023):           # both loops of the column update: few rows, and more than a wave's
        assert any(c.d == d and c.batch >= 64 for c in exact) and any(c.d == d and c.batch <= 3 for c in exact)
    assert {1023, 1024, 1025, 2050} <= set(F.SGD_D) and {63, 64, 65} <= set(F.SGD_D)
    lex = [c for c in F.LSVRG_CASES if c.kind == "exact"]
    assert {c.d for c in lex} == set(F.LSVRG_D) and {255, 256, 257} <= set(F.LSVRG_D) and {1, 63, 1025} <= set(F.LSVRG_D)
    assert {c.n for c in lex} == set(F.LSVRG_N) | {F.BIG_N} and {1, 2} <= set(F.LSVRG_N)
    big = [c for c in lex if c.n == F.BIG_N]
    assert F.BIG_N > 4096 * 256 and big and all(c.d in (1, 3) and c.steps == (1,) for c in big)
    assert {s for c in lex for s in c.steps} >= {0, 1, 100}
    assert any(c.steps[0] == 0 and len(c.steps) == 2 for c in lex)          # steps = 0, then an epoch on the same handle
    assert any(c.weights == "ehrm" and c.n >= 257 for c in lex) and any(c.reg == "l1" for c in lex)
    assert len({c.id for c in F.SGD_CASES + F.LSVRG_CASES}) == len(F.SGD_CASES) + len(F.LSVRG_CASES)
