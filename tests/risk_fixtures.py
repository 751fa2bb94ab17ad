"""Prescribed scores for the numbers a user reads - the logged objective sum_k sigma_k loss(v_(k)), the accuracy, the
fairness statistics - and their exact answers (a helper, no tests; test_risk_host.py pins on a CPU what every fixture
claims, test_gpu_risk.py feeds them to the device).

The reference.  risk_exact: the losses in float64 with the oracle's stable forms (oracle/prox.py: softplus; max(1 + v, 0)
and its square), sorted, math.fsum of sigma_k * loss_(k) with sigma from oracle/weights.py; erm: fsum(loss) / n.  With r
(a relabelled handle, r = y_own * y_owner) the losses are taken at r * v.

The patterns.  The sort-free risk (zband.hip: k_zb_risk, k_zb_risk_finish) selects the key at the last rank of every
band of equal weights, skips the elements tied with such a key in its pass and adds them back by count.  The tie
patterns are therefore laid out in RANK space around the family's actual band edges, which are recomputed here from
sigma the way the library's setup does (positions where sigma changes); families without bands (extremile, esrm, ehrm,
erm: the controls on the sort and the mean) get the nominal edges n // 3 - 1 and 2 n // 3 - 1.  A pattern with one case
per edge (or per band start) takes `case`; ncases() says how many there are."""
import math

import numpy as np

from oracle import prox, weights

BCE, HINGE, SQ = LOSSES = ["binary_cross_entropy", "hinge", "squared_hinge"]
BAR = 1e-12                                   # test_objective_golden_g7, test_objective_and_accuracy: the objective's bar

# family -> (weight_function, args as a function of n, B)
FAMILIES = {
    "superq_0.5": ("superquantile", lambda n: [0.5], None),
    "superq_0.37": ("superquantile", lambda n: [0.37], None),
    "aorr_0.2_0.8": ("aorr", lambda n: [0.2, 0.8], None),
    "aorr_0.13_0.71": ("aorr", lambda n: [0.13, 0.71], None),
    "aorr_dc": ("aorr_dc", lambda n: [(6 * n) // 10, n // 10], None),
    "extremile": ("extremile", lambda n: [2.0], None),
    "esrm": ("esrm", lambda n: [1.0], None),
    "ehrm": ("ehrm", lambda n: None, -5.0),
    "erm": ("erm", lambda n: None, None),
}
BANDED = ["superq_0.5", "superq_0.37", "aorr_0.2_0.8", "aorr_0.13_0.71", "aorr_dc"]
SMOOTH = ["extremile", "esrm", "ehrm"]
SIZES = [16, 17, 19, 1000, 4099, 70001]


def family(name, n):
    """-> (weight_function, args, B)"""
    wf, fa, B = FAMILIES[name]
    return wf, fa(n), B


def losses_of(name):
    return [BCE] if name == "ehrm" else LOSSES


# ------------------------------------------------------------------------------------------------------ reference
def sample_losses(loss, u):
    u = np.asarray(u, dtype=np.float64)
    if loss == BCE:
        return prox.softplus(u)
    t = np.maximum(1.0 + u, 0.0)
    if loss == HINGE:
        return t
    if loss == SQ:
        return t * t
    raise KeyError(loss)


def sigma_of(wf, args, n):
    return weights.get_weights(wf, n, args)[0]


def risk_exact(wf, args, loss, v, r=None):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    l = sample_losses(loss, v if r is None else np.asarray(r, dtype=np.float64) * v)
    if wf == "erm":
        return math.fsum(l) / l.size
    return math.fsum(sigma_of(wf, args, l.size) * np.sort(l))


# ------------------------------------------------------------------------------------------------------ band edges
def band_starts(wf, args, n):
    """first rank of every band of equal weights, and n (the positions where sigma changes); the nominal thirds for
    weights that are constant (erm) or change at every rank"""
    if wf != "erm":
        s = sigma_of(wf, args, n)
        pos = np.flatnonzero(s[1:] != s[:-1]) + 1
        if 1 <= pos.size <= 7:
            return [0] + [int(p) for p in pos] + [n]
    return [0, n // 3, (2 * n) // 3, n]


def edges(wf, args, n):
    """last rank of every band but the last"""
    return [s - 1 for s in band_starts(wf, args, n)[1:-1]]


# ------------------------------------------------------------------------------------------------------- patterns
PATTERNS = ["gaussian", "all_equal", "two_values", "span_one_edge", "span_all_edges", "ends_on_edge", "starts_after_edge",
            "dup33", "signed_zeros", "hinge_plateau", "extremes", "descending", "ascending"]
PER_EDGE = {"span_one_edge": 1, "ends_on_edge": 1, "starts_after_edge": 1, "signed_zeros": 2}
EXTREMES = [745.0, -745.0, 1e6, -1e6, 5e-324, -5e-324, 2.2e-308, -2.2e-308]
TWO = (-0.5, 1.25)


def ncases(name, n, wf, args):
    if name == "two_values":
        return 3 * (len(band_starts(wf, args, n)) - 2)
    return PER_EDGE.get(name, 0) * len(edges(wf, args, n)) or 1


def layout(name, n, wf, args, case=0):
    """-> [a, b): the sorted positions of the pattern's tie group (two_values: of its lower value); None: no group"""
    ed = edges(wf, args, n)
    clip = lambda a, b: (max(0, a), min(n, b))
    if name == "all_equal":
        return 0, n
    if name == "two_values":
        start = band_starts(wf, args, n)[1 + case // 3]
        return 0, min(max(start + case % 3 - 1, 1), n - 1)
    if name == "span_one_edge":
        return clip(ed[case] - 3, ed[case] + 6)                  # begins 3 ranks before the edge, ends 5 after it
    if name == "span_all_edges":
        return max(1, ed[0] - 2), min(n - 1, ed[-1] + 3)         # a distinct value on either side
    if name == "ends_on_edge":
        return clip(ed[case] - 4, ed[case] + 1)
    if name == "starts_after_edge":
        return clip(ed[case] + 1, ed[case] + 6)
    if name == "signed_zeros":
        return clip(ed[case // 2] - 3, ed[case // 2] + 6)
    return None


def zero_split(n, wf, args, case):
    """signed_zeros: the first sorted position of the +0.0 (the -0.0 come first).  Even cases: the -0.0 reach two ranks
    past the edge (the edge's key is -0.0, tied on both sides); odd cases: the last -0.0 IS the edge's rank, the first
    +0.0 the next band's first - two distinct keys with one loss"""
    e = edges(wf, args, n)[case // 2]
    a, b = layout("signed_zeros", n, wf, args, case)
    return min(max(e + (3 if case % 2 == 0 else 1), a), b)


def pattern(name, n, family, args, seed=0, case=0):
    """the named n-vector v for weights (family = weight function, args); shuffled with the seed except descending /
    ascending"""
    wf = family
    rng = np.random.default_rng([seed, n, PATTERNS.index(name), case])
    g = rng.standard_normal(n)
    s = np.sort(g)
    assert np.all(s[1:] > s[:-1])
    grp = layout(name, n, wf, args, case)
    if name == "gaussian":
        return g
    if name == "ascending":
        return s.copy()
    if name == "descending":
        return s[::-1].copy()
    if name == "all_equal":
        return np.full(n, 0.3)
    if name == "two_values":
        s = np.full(n, TWO[1])
        s[:grp[1]] = TWO[0]
    elif name in ("span_one_edge", "span_all_edges", "ends_on_edge", "starts_after_edge"):
        s[grp[0]:grp[1]] = s[grp[0]]
    elif name == "dup33":
        s = np.repeat(g[:(n + 32) // 33], 33)[:n].copy()
    elif name == "signed_zeros":
        a, b = grp
        z = zero_split(n, wf, args, case)
        mag = np.abs(g) + 2.0 ** -20
        s = np.concatenate((-np.sort(mag[:a])[::-1], np.full(z - a, -0.0), np.full(b - z, 0.0), np.sort(mag[b:])))
    elif name == "hinge_plateau":
        k = (9 * n) // 10                                        # 90 % at or below the kink: one loss (0), many keys
        s = np.concatenate((-1.0 - np.abs(g[:k]), -1.0 + np.abs(g[k:])))
        s[:k:10] = -1.0
    elif name == "extremes":
        s = g.copy()
        s[:len(EXTREMES)] = EXTREMES
    else:
        raise KeyError(name)
    return np.ascontiguousarray(rng.permutation(s))


def cases(n, wf, args, names=PATTERNS):
    """[(name, case)] of every pattern and case at this size"""
    return [(nm, c) for nm in names for c in range(ncases(nm, n, wf, args))]


def group_of(v, pos):
    """[a, b): the sorted positions (ascending KEY order: -0.0 before +0.0) holding the value at sorted position pos"""
    key = np.sort(flip_keys(v))
    return int(np.searchsorted(key, key[pos], "left")), int(np.searchsorted(key, key[pos], "right"))


def flip_keys(v):
    """the order-preserving uint64 image of a float64 the sorts and the select work on (device_math.h: flip_key)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    return np.where(b & top != 0, ~b, b | top)


# --------------------------------------------------------------------------------------------- scores, labels, groups
SCORES = ["gaussian", "on_threshold", "extreme"]
THRESHOLDS = [0.5, 0.3, 0.8]
GAP = 1e-6                                     # no score this close to a logit(threshold) unless it is exactly 0
ON_THRESHOLD = 3                               # rows per (sign of zero, label)
GROUPS = ["binary", "with_twos", "no_group0", "no_group1"]


def logit(t):
    return math.log(t / (1.0 - t))


def scores(name, n, seed=0):
    """-> (x.w, y): n scores and labels +-1.
    gaussian      3 N(0, 1), every |x.w - logit(thr)| >= GAP for thr in THRESHOLDS.
    on_threshold  the same, its first 4 * ON_THRESHOLD rows x.w = +0.0 / -0.0 under y = +1 / -1 (sigmoid = 0.5 exactly:
                  on the threshold 0.5, predicted +1 by calculate_acc.py and fair_metric.py alike), shuffled.
                  (a score in (-1.1e-16, 0) also rounds to sigmoid = 0.5 in the reference while the library compares
                  x.w with logit(threshold) = 0: scores that close to a threshold, other than the zeros, are not drawn).
    extreme       gaussian plus +-745 and +-1e6 under both labels (accuracy only: a probability of 0 has no Theil term)"""
    rng = np.random.default_rng([seed, n, SCORES.index(name)])
    x = 3.0 * rng.standard_normal(n)
    for t in THRESHOLDS:
        near = np.abs(x - logit(t)) < GAP
        x[near] = logit(t) + 2.0 * GAP
    y = np.where(rng.random(n) < 0.45, -1.0, 1.0)
    if name == "on_threshold":
        k = ON_THRESHOLD
        x[:4 * k] = np.repeat([0.0, -0.0, 0.0, -0.0], k)
        y[:4 * k] = np.repeat([1.0, 1.0, -1.0, -1.0], k)
    elif name == "extreme":
        x[:8] = [745.0, -745.0, 1e6, -1e6] * 2
        y[:8] = [1.0] * 4 + [-1.0] * 4
    elif name != "gaussian":
        raise KeyError(name)
    p = rng.permutation(n)
    return np.ascontiguousarray(x[p]), np.ascontiguousarray(y[p])


def relabel(y, seed=0):
    """labels of a borrower: a third of the rows flipped"""
    rng = np.random.default_rng([seed, y.size, 77])
    return np.where(rng.random(y.size) < 1.0 / 3.0, -y, y)


def groups(name, n, seed=0):
    """the group vector: 0 / 1 (binary); a few entries 2.0, which belong to neither group and stay in the Theil sums
    (with_twos); every row in group 1 / in group 0 (no_group0 / no_group1: the other group is empty)"""
    rng = np.random.default_rng([seed, n, 55 + GROUPS.index(name)])
    g = np.where(rng.random(n) < 0.4, 1.0, 0.0)
    if name == "with_twos":
        g[rng.choice(n, size=max(2, n // 50), replace=False)] = 2.0
    elif name == "no_group0":
        g[:] = 1.0
    elif name == "no_group1":
        g[:] = 0.0
    elif name != "binary":
        raise KeyError(name)
    return g


def _probs(xw):
    """sigmoid in the two-branch form of calculate_acc.py:6-8 / fair_metric.py:5-7"""
    xw = np.asarray(xw, dtype=np.float64)
    e = np.exp(-np.abs(xw))
    return np.where(xw >= 0, 1.0 / (1.0 + e), e / (e + 1.0))


def accuracy_ref(xw, y, threshold=0.5, loss=BCE):
    """calculate_acc.py:3-19 on given scores; squared_hinge (not a loss of the reference): predict +1 iff x.w >= 0"""
    y = np.asarray(y).reshape(-1)
    if loss == BCE:
        pred = np.where(_probs(xw) >= threshold, 1, -1)
    elif loss == HINGE:
        pred = np.ones(y.size, dtype=np.int64)           # calculate_acc.py:13-15 maps both outcomes to +1
    else:
        pred = np.where(np.asarray(xw) >= 0.0, 1, -1)
    return float(np.mean(pred == y))


def fair_ref(xw, y, group, threshold=0.5):
    """fair_metric.py:3-41 on given scores -> (SPD, DI, EOD, AOD, TI, FNRD).  The counts are exact; the Theil index is
    formed from fsum(b) and fsum(b log b) the way the library's host code combines its two sums."""
    prob = _probs(xw)
    pred = prob >= threshold
    pos = np.asarray(y).reshape(-1) > 0
    group = np.asarray(group).reshape(-1)
    cnt = lambda mask: np.float64(np.count_nonzero(mask))
    with np.errstate(divide="ignore", invalid="ignore"):
        P, TP, FN, TN, FP = [], [], [], [], []
        for gv in (0, 1):
            g = group == gv
            P.append(cnt(g & pred) / cnt(g))
            TP.append(cnt(g & pred & pos))
            FN.append(cnt(g & ~pred & pos))
            TN.append(cnt(g & ~pred & ~pos))
            FP.append(cnt(g & pred & ~pos))
        SPD = P[1] - P[0]
        DI = np.float64(np.inf) if P[0] == 0 else P[1] / P[0]
        TPR = [TP[k] / (TP[k] + FN[k]) for k in (0, 1)]
        FPR = [FP[k] / (FP[k] + TN[k]) for k in (0, 1)]
        FNR = [FN[k] / (TP[k] + FN[k]) for k in (0, 1)]
        EOD = TPR[1] - TPR[0]
        AOD = 0.5 * (FPR[1] - FPR[0] + EOD)
        b = prob - pos.astype(np.float64) + 1.0
        n = float(b.size)
        sb, sbl = math.fsum(b), math.fsum(b * np.log(b))
        mu = sb / n
        TI = (sbl - math.log(mu) * sb) / mu / n
    return tuple(float(x) for x in (SPD, DI, EOD, AOD, TI, FNR[1] - FNR[0]))
