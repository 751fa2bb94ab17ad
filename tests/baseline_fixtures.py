"""Prescribed epochs for the competitor baselines (csrc/baselines.hip: k_bl_sgd_epoch, k_bl_losses, k_bl_rank_coef,
k_bl_lsvrg_steps) - a helper, no tests; NumPy only.  test_baselines_host.py pins on a CPU what every fixture claims,
test_gpu_baselines_kernels.py feeds them to the device through _baselines.Baseline, one kernel epoch per call.

A case is a Problem (X, labels, loss, regulariser) and a list of ops on one handle: SetW, Sgd (one rbl_bl_sgd_epoch),
Lsvrg (one rbl_bl_lsvrg_epoch).  run_oracle plays the ops through oracle/baselines.py in float64, run_exact through
the restatement in fractions.Fraction below (hinge only).

Exact fixtures.  Hinge loss, X integer in [-3, 3], labels in {0, 1}, w0 integer, lr = 2^-3, dyadic weights
(k + 1) / 2^q strictly increasing in the rank k (EHRM: betas (2 k + 3) / 2^q, lossB = 1), l2_reg = n and l1_reg = n / 2
(so l2 w / n and the float32 term res * l1 / (2 n) only scale by powers of two; for a power of two n both are powers
of two), rands 0.25 / 0.75 (rnd * 2 - 1 = -+0.5).  Every product and sum of an epoch is then a dyadic rational
that fits a float64, whatever the order of the sums and whether or not a product is fused into its sum: the device
must equal the oracle bit for bit.  run_exact proves it per fixture: it returns the exact w and, in stats["bits"], the
largest log2(sum of |terms| * common denominator) over every sum it forms - below 53, every partial sum in any order
is representable.  Planted in the rows 0-4 (in the first mini-batch of an SGD epoch), against w0 = (1, 1, 0, ...):
  row 0  e0, y = 1       x.w0 = 1: the hinge tie 1 - y z = 0 (derivative -y / 2), loss 0
  row 1  2 e0, y = 1     loss 0 too, derivative 0: ties with row 0 - which of the two takes the larger weight is the
                         stable order's business (strictly increasing weights make it visible in w)
  row 2  e0 - e1, y = 1  x.w0 = 0: loss 1 == lossB with derivative -1 (EHRM: alpha, not beta); d >= 2
  row 3  y = 0           loss exactly 1 whatever x: ties with row 2, derivative 0
  row 4  -e0, y = 1      loss 2 > lossB (EHRM: beta)
and w0[2] = 0 (d >= 3): a zero coordinate for the l1 term at step 0.

Smooth fixtures.  BCE on oracle/problems.py: make_problem data rounded to multiples of 2^-8, compared under the
baselines' bound of test_gpu_baselines.py, BOUND * max(1, max|ref|).  Their w0 is a plain Gaussian draw, not rounded: a
dyadic w0 puts every x.w on a grid, rows with opposite labels and opposite x.w then have mathematically equal BCE losses,
softplus(z) - z against softplus(-z), and which of the two computed values is the smaller hangs on the last bit of log1p
and exp - where the device's library and NumPy's differ, so that the two sides rank such rows differently.  (Measured with
w0 in multiples of 2^-6: 17 and 129 such pairs at n = 4099 moved w by 6e-7 and 6e-8, against a bound of 1e-10; no
kernel is wrong there, the order is not defined.)  near_ties counts such pairs; the host test holds it at zero."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle import baselines as ob
from oracle import problems

HINGE, BCE = "hinge", "binary_cross_entropy"
BOUND = 1e-10                                  # test_gpu_baselines.py: the device sums a mini-batch's rows in a fixed order, BLAS in another
LR = 0.125
BIG_N = (1 << 20) + 257                        # k_bl_losses / k_bl_rank_coef: 4096 blocks of 256 take a second trip

SgdCase = namedtuple("SgdCase", "id kind d batch steps weights reg")
LsvrgCase = namedtuple("LsvrgCase", "id kind d n steps uniform weights reg samples")     # steps: one entry per epoch
Problem = namedtuple("Problem", "X y01 w0 loss lr l2 l1 lossB")
SetW = namedtuple("SetW", "w")
Sgd = namedtuple("Sgd", "order steps batch ab bb rands")
Lsvrg = namedtuple("Lsvrg", "alphas betas samples uniform rands")


def _sgd(kind, d, batch, steps, weights, reg):
    return SgdCase(f"{kind}-d{d}-b{batch}-s{steps}-{weights}-{reg}", kind, d, batch, steps, weights, reg)


def _lsvrg(kind, d, n, steps, uniform, weights, reg, samples="rng"):
    sid = "+".join(str(s) for s in steps)
    return LsvrgCase(f"{kind}-d{d}-n{n}-s{sid}-u{uniform}-{weights}-{reg}-{samples}", kind, d, n, tuple(steps), uniform,
                     weights, reg, samples)


SGD_D = [1, 3, 63, 64, 65, 130, 1023, 1024, 1025, 2050]
SGD_BATCH = [1, 2, 3, 5, 6, 7, 8, 9, 12, 63, 64, 65, 67, 1023, 1024]      # (6, 12: tails 6 and 4 of the 8-row accumulation)
SGD_CASES = [
    _sgd("exact", 1, 1, 5, "inc", "none"),
    _sgd("exact", 1, 1024, 3, "inc", "none"),
    _sgd("exact", 3, 2, 5, "inc", "l1"),
    _sgd("exact", 3, 1023, 3, "ehrm", "l1"),
    _sgd("exact", 63, 3, 4, "ehrm", "l2"),
    _sgd("exact", 64, 5, 4, "inc", "l2"),
    _sgd("exact", 65, 7, 4, "ehrm", "none"),
    _sgd("exact", 130, 8, 3, "inc", "l1"),
    _sgd("exact", 130, 9, 5, "ehrm", "none"),
    _sgd("exact", 3, 6, 4, "ehrm", "none"),
    _sgd("exact", 65, 12, 3, "inc", "l2"),
    _sgd("exact", 63, 63, 3, "inc", "none"),
    _sgd("exact", 65, 65, 3, "ehrm", "l1"),
    _sgd("exact", 130, 67, 3, "inc", "l2"),
    _sgd("exact", 64, 1024, 3, "ehrm", "none"),
    _sgd("exact", 1023, 64, 3, "inc", "none"),
    _sgd("exact", 1023, 1, 5, "inc", "l1"),
    _sgd("exact", 1024, 65, 3, "ehrm", "l2"),
    _sgd("exact", 1024, 2, 4, "inc", "none"),
    _sgd("exact", 1025, 67, 3, "inc", "l1"),
    _sgd("exact", 1025, 3, 4, "ehrm", "none"),
    _sgd("exact", 2050, 64, 3, "ehrm", "none"),
    _sgd("exact", 2050, 3, 5, "inc", "l2"),
    _sgd("smooth", 1, 1, 5, "inc", "l2"),
    _sgd("smooth", 3, 3, 5, "ehrm", "none"),
    _sgd("smooth", 3, 7, 5, "inc", "l1"),
    _sgd("smooth", 64, 8, 4, "ehrm", "none"),
    _sgd("smooth", 65, 9, 4, "inc", "l1"),
    _sgd("smooth", 130, 63, 3, "ehrm", "l2"),
    _sgd("smooth", 130, 5, 5, "inc", "none"),
    _sgd("smooth", 63, 1023, 3, "ehrm", "none"),
    _sgd("smooth", 64, 1024, 3, "inc", "l2"),
    _sgd("smooth", 1023, 2, 4, "inc", "l2"),
    _sgd("smooth", 1023, 65, 3, "ehrm", "none"),
    _sgd("smooth", 1024, 64, 3, "inc", "none"),
    _sgd("smooth", 1025, 65, 3, "ehrm", "l1"),
    _sgd("smooth", 2050, 67, 3, "inc", "l2"),
    _sgd("smooth", 2050, 1, 5, "inc", "none"),
]

LSVRG_D = [1, 3, 63, 255, 256, 257, 1025]
LSVRG_N = [1, 2, 257, 4099]
LSVRG_CASES = [
    _lsvrg("exact", 1, 1, [1], 1, "inc", "none"),
    _lsvrg("exact", 3, 1, [100], 0, "inc", "l1"),
    _lsvrg("exact", 3, 2, [100], 0, "inc", "none", "repeat"),
    _lsvrg("exact", 63, 2, [1], 1, "ehrm", "none"),
    _lsvrg("exact", 3, 257, [0, 100], 0, "inc", "none"),
    _lsvrg("exact", 63, 257, [0, 1], 1, "ehrm", "l1"),
    _lsvrg("exact", 255, 257, [100], 1, "inc", "none", "repeat"),
    _lsvrg("exact", 256, 257, [100], 0, "ehrm", "l1"),
    _lsvrg("exact", 257, 257, [5], 1, "ehrm", "l2"),
    _lsvrg("exact", 257, 257, [100, 100], 1, "inc", "none"),
    _lsvrg("exact", 1025, 257, [100], 0, "inc", "none", "repeat"),
    _lsvrg("exact", 1025, 257, [1], 1, "ehrm", "l2"),
    _lsvrg("exact", 3, 4099, [100], 0, "inc", "l1", "repeat"),
    _lsvrg("exact", 63, 4099, [100], 1, "ehrm", "none"),
    _lsvrg("exact", 1, 4099, [1], 0, "inc", "l2"),
    _lsvrg("exact", 3, BIG_N, [1], 0, "inc", "none"),
    _lsvrg("smooth", 1, 1, [100], 0, "inc", "l2"),
    _lsvrg("smooth", 3, 2, [100], 1, "inc", "none"),
    _lsvrg("smooth", 3, 257, [100], 1, "inc", "l2", "repeat"),
    _lsvrg("smooth", 63, 257, [100], 1, "ehrm", "none"),
    _lsvrg("smooth", 256, 257, [1], 1, "inc", "l1"),
    _lsvrg("smooth", 1025, 257, [100], 0, "inc", "l1"),
    _lsvrg("smooth", 3, 4099, [100, 100], 0, "ehrm", "l2", "repeat"),
    _lsvrg("smooth", 255, 4099, [0, 100], 0, "inc", "l2"),
    _lsvrg("smooth", 257, 4099, [100], 1, "ehrm", "l1"),
]


# ------------------------------------------------------------------------------------------------------- builders
def _seed(case):
    return [len(case.id)] + [ord(c) for c in case.id]


def dyadic_weights(m, ehrm):
    """(k + 1) / 2^q, q = 2 ceil(log2 m): strictly increasing, sum in (1/8, 1/2]; EHRM: betas (2 k + 3) / 2^q as well"""
    q = 2 * max(1, math.ceil(math.log2(m)))
    k = np.arange(m, dtype=np.float64)
    return (k + 1.0) / 2.0 ** q, ((2.0 * k + 3.0) / 2.0 ** q if ehrm else None)


def _regs(reg, n):
    return (float(n) if reg == "l2" else 0.0), (n / 2.0 if reg == "l1" else 0.0)


def rands_for(reg, steps):
    return np.where(np.arange(steps) % 2 == 0, 0.25, 0.75).astype(np.float32) if reg == "l1" else None


def _exact_data(rng, n, d):
    """-> X, y01, w0 with the planted rows of the module docstring in rows 0 .. min(n, 5) - 1"""
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    y01 = rng.integers(0, 2, size=n).astype(np.float64)
    w0 = rng.integers(-1, 2, size=d).astype(np.float64)
    w0[:3] = [1.0, 1.0, 0.0][:d]
    e = np.eye(d)
    planted = [(e[0], 1.0), (2.0 * e[0], 1.0), (e[0] - e[1], 1.0) if d >= 2 else (None, 0.0), (None, 0.0), (-e[0], 1.0)]
    for r, (x, yy) in enumerate(planted[:n]):
        if x is not None:
            X[r] = x
        y01[r] = yy
    return X, y01, w0


def _smooth_data(rng, n, d, seed, l1):
    """X rounded to multiples of 2^-8; w0 is NOT rounded (module docstring: near ties)"""
    Xs, y = problems.make_problem(max(n, 64), d, seed=seed)
    X = np.ascontiguousarray(np.round(Xs[:n] * 256.0) / 256.0)
    w0 = rng.standard_normal(d) / math.sqrt(d)
    if l1:
        w0[::3] = 0.0
    return X, ob.labels01(y[:n]), w0


def near_ties(P, ops, ulps=8):
    """along the oracle's trajectory, at every LSVRG checkpoint and every SGD step: pairs of sorted neighbours whose losses
    differ by no more than `ulps` units in the last place (equal ones included: no smooth fixture has two equal rows)"""
    count, w = 0, np.zeros(P.X.shape[1])
    for op in ops:
        if isinstance(op, Sgd):
            for s in range(op.steps):
                w_s = run_oracle(P, [SetW(w), op._replace(steps=s)])[1] if s else w
                rows = op.order[s * op.batch:(s + 1) * op.batch]
                l = np.sort(ob.sample_losses(P.loss, P.X[rows] @ w_s, P.y01[rows]))
                count += int(np.count_nonzero(np.diff(l) <= ulps * np.spacing(l[1:])))
        elif isinstance(op, Lsvrg):
            l = np.sort(ob.sample_losses(P.loss, P.X @ w, P.y01))
            count += int(np.count_nonzero(np.diff(l) <= ulps * np.spacing(l[1:])))
        w = run_oracle(P, [SetW(w), op])[1] if not isinstance(op, SetW) else np.array(op.w, dtype=np.float64)
    return count


def sgd_problem(case):
    """-> Problem, ops: n the next power of two >= steps * batch + 5; the order is a strict subset of the rows, unsorted,
    without repeats, the planted rows among its first `batch`"""
    rng = np.random.default_rng(_seed(case))
    cnt = case.steps * case.batch
    n = 1 << (cnt + 5 - 1).bit_length()
    exact = case.kind == "exact"
    ehrm = case.weights == "ehrm"
    if exact:
        X, y01, w0 = _exact_data(rng, n, case.d)
        l2, l1 = _regs(case.reg, n)
    else:
        X, y01, w0 = _smooth_data(rng, n, case.d, 700 + case.d + case.batch, case.reg == "l1")
        l2, l1 = (1.0 if case.reg == "l2" else 0.0), (1.0 if case.reg == "l1" else 0.0)
    k = min(case.batch, 5)
    rest = rng.permutation(np.arange(k, n))[:cnt - k]
    order = np.concatenate((rng.permutation(np.concatenate((np.arange(k), rest[:case.batch - k]))), rest[case.batch - k:]))
    ab, bb = dyadic_weights(case.batch, ehrm)
    P = Problem(X, y01, w0, HINGE if exact else BCE, LR, l2, l1, (1.0 if exact else 0.69) if ehrm else None)
    return P, [SetW(w0), Sgd(order.astype(np.int32), case.steps, case.batch, ab, bb, rands_for(case.reg, case.steps))]


def _samples(rng, n, steps, kind):
    s = rng.integers(0, n, size=steps)
    if kind == "repeat" and steps >= 5:
        s[1:4] = s[1]                                       # the same sample three times in a row
    return s.astype(np.int32)


def lsvrg_problem(case):
    """-> Problem, ops: one Lsvrg per entry of case.steps, on one handle"""
    rng = np.random.default_rng(_seed(case))
    n, d = case.n, case.d
    exact = case.kind == "exact"
    ehrm = case.weights == "ehrm"
    if exact:
        X, y01, w0 = _exact_data(rng, n, d)
        l2, l1 = _regs(case.reg, n)
    else:
        X, y01, w0 = _smooth_data(rng, n, d, 900 + d + n, case.reg == "l1")
        l2, l1 = (1.0 if case.reg == "l2" else 0.0), (1.0 if case.reg == "l1" else 0.0)
    a, b = dyadic_weights(n, ehrm)
    P = Problem(X, y01, w0, HINGE if exact else BCE, LR, l2, l1, (1.0 if exact else 0.69) if ehrm else None)
    ops = [SetW(w0)] + [Lsvrg(a, b, _samples(rng, n, s, case.samples), case.uniform, rands_for(case.reg, s)) for s in case.steps]
    return P, ops


def sequence_problem():
    """one handle through: an SGD epoch with a small steps * batch, a larger one (the index buffers regrow), an LSVRG epoch
    of 100 steps, set_w to a prescribed w, another SGD epoch.  Exact fixture, l1 with its rands."""
    rng = np.random.default_rng(4242)
    n, d = 512, 65
    X, y01, w0 = _exact_data(rng, n, d)
    l2, l1 = _regs("l1", n)
    P = Problem(X, y01, w0, HINGE, LR, l2, l1, None)
    ops = [SetW(w0)]
    for steps, batch in ((3, 5), (4, 67)):
        ab, _ = dyadic_weights(batch, False)
        ops.append(Sgd(rng.permutation(n)[:steps * batch].astype(np.int32), steps, batch, ab, None, rands_for("l1", steps)))
    a, _ = dyadic_weights(n, False)
    ops.append(Lsvrg(a, None, _samples(rng, n, 100, "repeat"), 1, rands_for("l1", 100)))
    ops.append(SetW(rng.integers(-2, 3, size=d).astype(np.float64)))
    ab, _ = dyadic_weights(9, False)
    ops.append(Sgd(rng.permutation(n)[:27].astype(np.int32), 3, 9, ab, None, rands_for("l1", 3)))
    return P, ops


# ----------------------------------------------------------------------------------------------- float64 reference
def run_oracle(P, ops):
    """-> w after every op, through oracle/baselines.py"""
    w, out = np.zeros(P.X.shape[1]), []
    for op in ops:
        if isinstance(op, SetW):
            w = np.array(op.w, dtype=np.float64)
        elif isinstance(op, Sgd):
            w = ob.sgd_epoch(P.X, P.y01, w, P.loss, P.lr, op.order, op.batch, op.steps, op.ab, op.bb, P.lossB, P.l2, P.l1,
                             op.rands)
        else:
            w = ob.lsvrg_epoch(P.X, P.y01, w, P.loss, P.lr, op.samples, bool(op.uniform), op.alphas, op.betas, P.lossB,
                               P.l2, P.l1, op.rands)
        out.append(np.array(w))
    return out


# ------------------------------------------------------------------- the two hinge epochs in exact rational arithmetic
def _fr(a):
    return [Fraction(float(v)) for v in a]


def _dloss(t, yi, mut):
    """hinge derivative in z at t = 1 - y z; the tie t == 0 takes half (torch.maximum splits the gradient)"""
    return Fraction(-yi) if t > 0 else Fraction(-yi, 1 if mut == "kink" else 2) if t == 0 else Fraction(0)


def _coef(z, y, wa, wb, lossB, st, mut):
    """hinge losses, their stable order, coefficient c_i = weight(rank i) * loss_i'.  The losses are sorted as integers:
    multiples of the reciprocal of their common (power of two) denominator"""
    b = len(z)
    t = [1 - zi if yi else 1 for zi, yi in zip(z, y)]                    # labels are 0 or 1
    D = max(getattr(ti, "denominator", 1) for ti in t)
    assert D & (D - 1) == 0
    key = [max(ti.numerator * (D // ti.denominator), 0) if yi else D for ti, yi in zip(t, y)]
    order = sorted(reversed(range(b)) if mut == "ties" else range(b), key=key.__getitem__)      # sorted() is stable
    kB = None if wb is None else lossB * D
    c, prev = [Fraction(0)] * b, None
    for k, i in enumerate(order):
        ki = key[i]
        st["ties"] += ki == prev
        prev = ki
        if kB is not None:
            st["sides"] |= 1 if ki < kB else 2 if ki > kB else 0
        if y[i]:
            c[i] = (wa[k] if kB is None or ki <= kB else wb[k]) * _dloss(t[i], 1, mut)
            st["t0"] += t[i] == 0
            st["onB"] += ki == kB
    return c, order


def _reg(wj, P, n, rnd):
    g = Fraction(0)
    if P.l2:
        g += Fraction(P.l2) * wj / n
    if P.l1:
        g += (1 if wj > 0 else -1 if wj < 0 else 2 * rnd - 1) * Fraction(P.l1) / (2 * n)
    return g


def _bits(st, mag, *dens):
    """a sum whose |terms| add up to mag, every term a multiple of 1 / max(dens)"""
    if mag > 0:
        st["bits"] = max(st["bits"], math.log2(float(mag) * max(dens)))


def _scaled(v):
    """-> (integers, D) with v_k = integers[k] / D, D the (power of two) common denominator: the sums below run on Python
    integers, which is exact rational arithmetic all the same"""
    D = max(x.denominator for x in v)
    assert D & (D - 1) == 0
    return [x.numerator * (D // x.denominator) for x in v], D


def _rows(X, rows, w, st):
    """x_i . w for the given rows"""
    Xr = X[rows]
    wi, D = _scaled(w)
    _bits(st, float(np.max(np.abs(Xr) @ np.abs(np.array([float(x) for x in w])))) * 1.0001, D)
    return [Fraction(sum(x * wj for x, wj in zip(r, wi) if x), D) for r in Xr.astype(np.int64).tolist()]


def _cols(X, rows, c, st):
    """sum_i c_i x_i over the given rows"""
    Xr = X[rows]
    ci, D = _scaled(c)
    _bits(st, float(np.max(np.abs(np.array([float(x) for x in c])) @ np.abs(Xr))) * 1.0001, D)
    g = [0] * Xr.shape[1]
    for cc, r in zip(ci, Xr.astype(np.int64).tolist()):
        if cc:
            g = [gj + x * cc for gj, x in zip(g, r)]
    return [Fraction(gj, D) for gj in g]


def _step(w, direction, P, n, rnd, st):
    """w - lr (direction + regulariser); the sums of a coordinate's update and the product l2 w_j are bounded as well"""
    lr, out, mag, den = Fraction(P.lr), [], Fraction(0), 1
    for wj, gj in zip(w, direction):
        a, r = lr * gj, lr * _reg(wj, P, n, rnd)
        out.append(wj - (a + r))
        mag = max(mag, abs(wj) * max(1, P.l2) + abs(a) + abs(r))
        den = max(den, wj.denominator, a.denominator, r.denominator)
    _bits(st, mag, den)
    return out


def run_exact(P, ops, mut=None):
    """-> (w after every op as lists of Fraction, stats).  mut: "ties" breaks loss ties by descending index, "kink" takes
    the derivative -y at the hinge tie - the wrong answers a fixture must tell from the right one.
    stats: bits (module docstring); t0, onB, ties: rows with y = 1 on the hinge tie / with loss == lossB, and sorted
    neighbours with equal losses, counted at the first step of an SGD epoch and at an LSVRG checkpoint; sides: 3 when losses
    lie on both sides of lossB; zeros: coordinates w_j = 0 under l1 at the first step; ndiff: LSVRG steps whose two
    derivatives differ"""
    assert P.loss == HINGE
    n = P.X.shape[0]
    y = [int(v) for v in P.y01]
    assert set(y) <= {0, 1}
    st = dict(bits=0.0, t0=0, onB=0, sides=0, ties=0, zeros=0, ndiff=0)
    scratch = dict(st)
    lossB = None if P.lossB is None else Fraction(P.lossB)
    w, out = [Fraction(0)] * P.X.shape[1], []
    for op in ops:
        if isinstance(op, SetW):
            w = _fr(op.w)
        elif isinstance(op, Sgd):
            ab, bb = _fr(op.ab), (None if op.bb is None else _fr(op.bb))
            for s in range(op.steps):
                rows = [int(i) for i in op.order[s * op.batch:(s + 1) * op.batch]]
                assert len(rows) == op.batch
                st["zeros"] += sum(1 for wj in w if wj == 0) if (P.l1 and s == 0) else 0
                z = _rows(P.X, rows, w, st)
                c, _ = _coef(z, [y[i] for i in rows], ab, bb, lossB, st if s == 0 else scratch, mut)
                w = _step(w, _cols(P.X, rows, c, st), P, n, Fraction(float(op.rands[s])) if P.l1 else 0, st)
        else:
            a, b = _fr(op.alphas), (None if op.betas is None else _fr(op.betas))
            rows = list(range(n))
            st["zeros"] += sum(1 for wj in w if wj == 0) if (P.l1 and len(op.samples)) else 0
            c, order = _coef(_rows(P.X, rows, w, st), y, a, b, lossB, st, mut)
            g_chk, w_chk = _cols(P.X, rows, c, st), list(w)
            for s, i in enumerate(int(v) for v in op.samples):
                row = i if op.uniform else order[i]
                z, zc = _rows(P.X, [row], w, st)[0], _rows(P.X, [row], w_chk, st)[0]
                dl = [_dloss(1 - y[row] * zz, y[row], mut) for zz in (z, zc)]
                scale = Fraction(1)
                if op.uniform:
                    use_b = b is not None and not max(1 - y[row] * z, 0) <= lossB
                    scale = n * ((b if use_b else a)[order[i] if mut == "uniform" else i])
                st["ndiff"] += int(dl[0] != dl[1])
                direction = [scale * (dl[0] - dl[1]) * int(x) + gj for x, gj in zip(P.X[row].tolist(), g_chk)]
                w = _step(w, direction, P, n, Fraction(float(op.rands[s])) if P.l1 else 0, st)
        out.append(list(w))
    return out, st


def equals_exact(w_float, w_exact):
    return len(w_float) == len(w_exact) and all(Fraction(float(a)) == b for a, b in zip(w_float, w_exact))
