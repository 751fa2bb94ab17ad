"""An extended-precision reference of the loss math of csrc/device_math.h, and the inputs it is run on (a helper, no
tests; used by test_lossmath_host.py on the CPU and test_gpu_lossmath.py on the device).

The reference shares neither the algorithm nor the precision of what it judges:
  BCE prox         the root of sigma sigmoid(x) + rho (x - m) by plain bisection on [m - sigma / rho, m] in np.longdouble
                   (80-bit), run until the midpoint repeats an end, then two Newton steps in the same type.  No
                   safeguarded Newton, no warm start, no series estimate.  test_lossmath_host.py certifies it against
                   mpmath at 50 digits.
  hinge, sq. hinge the closed forms, in fractions.Fraction (exact) and in longdouble for arrays.
  losses           softplus, sigmoid and the three sample losses in longdouble.

Every comparison against it is per element, |got - ref| <= bar * eps * scale(ref_i, m_i), eps = 2^-52,
scale = max(1, |x*|, |m|) (the hinge adds sigma / rho: its one subtraction rounds at that size).

Inputs: GRID and RANDOM (the element prox tables), EDGE_M (m for the other call sites), and the designs of the PAV and
EHRM cases, which test_lossmath_host.py validates on the CPU so that a failure on the device means the kernel."""
import math
from fractions import Fraction

import numpy as np

from oracle import weights

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, ("tests/lossmath_ref.py needs an 80-bit (or wider) np.longdouble: "
                                  f"this platform's has eps = {np.finfo(LD).eps}")
EPS = 2.0 ** -52
BCE, HINGE, SQ = LOSSES = ("binary_cross_entropy", "hinge", "squared_hinge")
BAR = {BCE: 16.0, HINGE: 0.0, SQ: 4.0}          # the device's element prox, in eps * scale (hinge: the same bits)
BAR_ORACLE = {BCE: 4.0, HINGE: 1.0, SQ: 2.0}    # the float64 restatements of oracle/ and tests/sqhinge_ref.py
BAR_PAV = 32.0                                   # a pooled block: BAR[BCE] + one rounding per mean, doubled


def ld(x):
    return np.asarray(x, dtype=LD)


# --------------------------------------------------------------------------------------------------- the functions
def sigmoid(x):
    x = ld(x)
    e = np.exp(-np.abs(x))
    return np.where(x > 0, 1 / (1 + e), e / (1 + e))


def softplus(x):
    x = ld(x)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sample_loss(loss, v):
    v = ld(v)
    if loss == BCE:
        return softplus(v)
    t = np.maximum(1 + v, 0)
    return t * t if loss == SQ else t


def prox_bce(sigma, rho, m, max_halvings=20000):
    """longdouble root of sigma sigmoid(x) + rho (x - m) per element: bisection to its fixed point, two Newton steps"""
    sigma, rho, m = np.broadcast_arrays(ld(sigma), ld(rho), ld(m))
    sigma, rho, m = sigma.reshape(-1), rho.reshape(-1), m.reshape(-1)
    g = lambda x, i: sigma[i] * sigmoid(x) + rho[i] * (x - m[i])
    lo, hi = m - sigma / rho, m.copy()             # g(lo) <= 0 <= g(hi) because 0 <= sigmoid <= 1
    act = np.flatnonzero(lo < hi)
    for _ in range(max_halvings):
        if act.size == 0:
            break
        mid = lo[act] + (hi[act] - lo[act]) / 2
        moved = (mid > lo[act]) & (mid < hi[act])
        act, mid = act[moved], mid[moved]
        neg = g(mid, act) < 0
        lo[act[neg]] = mid[neg]
        hi[act[~neg]] = mid[~neg]
    assert act.size == 0, "the bisection did not reach its fixed point"
    x = np.where(g(hi, slice(None)) <= -g(lo, slice(None)), hi, lo)
    for _ in range(2):
        s = sigmoid(x)
        x = x - (sigma * s + rho * (x - m)) / (sigma * s * (1 - s) + rho)
    return np.minimum(np.maximum(x, lo), hi)       # (a Newton step never leaves [lo, hi] by more than rounding)


def prox_hinge(sigma, rho, m):
    sigma, rho, m = ld(sigma), ld(rho), ld(m)
    a = m - sigma / rho
    return np.where(a >= -1, a, np.where(m <= -1, m, LD(-1)))


def prox_sqhinge(sigma, rho, m):
    sigma, rho, m = ld(sigma), ld(rho), ld(m)
    return np.where((m <= -1) | (sigma == 0), m, (rho * m - 2 * sigma) / (rho + 2 * sigma))


def prox(loss, sigma, rho, m):
    return {BCE: prox_bce, HINGE: prox_hinge, SQ: prox_sqhinge}[loss](sigma, rho, m)


def prox_fraction(loss, sigma, rho, m):
    """the exact hinge / squared hinge prox of float64 scalars, a Fraction"""
    s, r, m = Fraction(float(sigma)), Fraction(float(rho)), Fraction(float(m))
    if loss == HINGE:
        a = m - s / r
        return a if a >= -1 else (m if m <= -1 else Fraction(-1))
    assert loss == SQ
    return m if (m <= -1 or s == 0) else (r * m - 2 * s) / (r + 2 * s)


def ld_to_fraction(v):
    """a longdouble, exactly (also below the range of float64)"""
    mant, e = np.frexp(LD(v))
    hi = float(mant)
    return (Fraction(hi) + Fraction(float(mant - LD(hi)))) * Fraction(2) ** int(e)


def fraction_to_ld(q):
    hi = float(q)
    return LD(hi) + LD(float(q - Fraction(hi)))


def scale(x, m, sigma_over_rho=None):
    """max(1, |x*|, |m|) per element; the hinge passes sigma / rho as well"""
    s = np.maximum(np.maximum(np.abs(ld(x)), np.abs(ld(m))), 1)
    return s if sigma_over_rho is None else np.maximum(s, np.abs(ld(sigma_over_rho)))


def scale_of(loss, x, sigma, rho, m):
    return scale(x, m, ld(sigma) / ld(rho) if loss == HINGE else None)


def err_units(got, ref, sc):
    """|got - ref| in units of eps * scale, float64 per element (NaN / inf where got is not finite)"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.asarray(np.abs(ld(got) - ref) / (LD(EPS) * sc), dtype=np.float64)


# --------------------------------------------------------------------------------------------------- the element tables
# |m| <= 1e15 and sigma / rho <= 1e14: far beyond that rho * m and 2 sigma overflow in the squared hinge's closed form
# (rho m - 2 sigma) / (rho + 2 sigma); within it every product of the three forms stays below 1e36.
M_ABS = [1e-300, 1e-8, 0.5, 1.0, 6.0, 30.0, 36.5, 37.5, 40.0, 700.0, 745.2, 746.0, 1e6, 1e15]
GRID_M = np.array([0.0] + M_ABS + [-x for x in M_ABS])
GRID_RATIO = 10.0 ** np.arange(-12, 13, 2)
GRID_RHO = 2.0 ** np.arange(-40, 21, 12)
RHO_POW = (-40, 20)


def grid():
    """13 ratios x 6 rho x 29 m -> (sigma, rho, m), float64; sigma = fl(ratio * rho)"""
    ratio, rho, m = np.meshgrid(GRID_RATIO, GRID_RHO, GRID_M, indexing="ij")
    return (ratio * rho).reshape(-1), rho.reshape(-1).copy(), m.reshape(-1).copy()


def random_set(n=2500, seed=20240):
    """log-uniform sigma / rho in 1e-14 .. 1e14 and |m| in 1e-12 .. 1e15, 400 m in +-50 and 200 in +-760, rho a power
    of two in 2^-40 .. 2^20, every 25th sigma 0"""
    rng = np.random.default_rng(seed)
    ratio = 10.0 ** rng.uniform(-14, 14, n)
    rho = 2.0 ** rng.integers(RHO_POW[0], RHO_POW[1] + 1, n).astype(np.float64)
    m = 10.0 ** rng.uniform(-12, 15, n) * rng.choice([-1.0, 1.0], n)
    m[:400] = rng.uniform(-50, 50, 400)
    m[400:600] = rng.uniform(-760, 760, 200)
    sigma = ratio * rho
    sigma[::25] = 0.0
    p = rng.permutation(n)
    return sigma[p], rho[p], m[p]


def tables():
    """grid and random set in one: (sigma, rho, m)"""
    g, r = grid(), random_set()
    return tuple(np.concatenate([a, b]) for a, b in zip(g, r))


EDGE_LIST = [0.0] + [s * x for x in (36.5, 37.5, 700.0, 745.2, 746.0, 1e6, 1e-300) for s in (1.0, -1.0)]


def edge_m(n=None, seed=7):
    """the shared m of the other call sites: the edge values and 400 ordinary draws in +-50, shuffled; n: cut or tile to
    n entries (the first 15 are always the edge values)"""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.concatenate([np.array(EDGE_LIST[1:]), rng.uniform(-50, 50, 400)]))
    m = np.concatenate([np.array(EDGE_LIST), rest])
    if n is None:
        return m
    return np.resize(m, n).copy()


# --------------------------------------------------------------------------------------------------- PAV designs
# Everything is a multiple of 2^-20 of bounded size, so every prefix sum and prefix difference of sigma and of m is
# exact in 53 bits: the only rounding before a block's solve is the division of the two means.
DYADIC = 2.0 ** -20
PAV_RHO = (2.0 ** -22, 2.0 ** -4, 1.0)
PAV_ONE_BLOCK_N = (2, 64, 2047, 2048, 2049, 4097)
PAV_SEG_LEN = (1, 2, 3, 63, 64, 65, 2047, 2049)              # positions 198 .. 2244 are one segment: it straddles 2048
PAV_SEG_M = (-700.0, -37.5, -6.0, -0.5, 1.0, 7.0, 36.5, 700.0)
PAV_EQUAL_M = (0.5, -37.5, 36.5, -6.0, 700.0, 3.0)


def _sig_ramp(n):
    return 2.0 ** -3 + np.arange(n) * 2.0 ** -13              # strictly increasing; mean 1/4 at n = 2049


def pav_design(kind, n=None):
    """-> (sigma, m sorted, segment lengths).  "separate": constant sigma, strictly increasing m; "one_block": equal m,
    increasing sigma, n positions; "segments": PAV_SEG_LEN"""
    if kind == "separate":
        rng = np.random.default_rng(5)
        m = np.unique(np.concatenate([np.array([-746.0, -745.25, -700.0, -37.5, -36.5, 36.5, 37.5, 700.0, 745.25, 746.0]),
                                      rng.integers(-50 * 32, 50 * 32, 4000) / 32.0]))
        return np.full(m.size, 0.375), m, np.ones(m.size, dtype=np.int64)
    if kind == "one_block":
        return _sig_ramp(n), np.full(n, PAV_EQUAL_M[PAV_ONE_BLOCK_N.index(n)]), np.array([n])
    assert kind == "segments"
    sigma = np.concatenate([_sig_ramp(k) for k in PAV_SEG_LEN])
    m = np.concatenate([np.full(k, v) for k, v in zip(PAV_SEG_LEN, PAV_SEG_M)])
    return sigma, m, np.array(PAV_SEG_LEN)


def pav_reference(loss, sigma, rho, m, seg):
    """per segment the prox at (mean sigma, mean m), the means in longdouble -> (per position, per segment), and the
    scale per position"""
    ends = np.cumsum(seg)
    starts = ends - seg
    S = np.array([np.sum(ld(sigma[a:b])) / (b - a) for a, b in zip(starts, ends)], dtype=LD)
    M = np.array([np.sum(ld(m[a:b])) / (b - a) for a, b in zip(starts, ends)], dtype=LD)
    x = prox(loss, S, LD(rho), M)
    sc = scale_of(loss, x, S, LD(rho), M)
    return np.repeat(x, seg), x, np.repeat(sc, seg)


def pav_strict_segments(loss, sigma, rho, m, seg):
    """per segment: do its element values decrease from each position to the next by more than the device's rounding
    (4 BAR_PAV eps scale)?  Then every merge the device makes joins exactly two blocks and a segment of k positions
    costs k - 1 of them; where values tie (the flat side of a loss) the device need not merge at all"""
    x = prox(loss, sigma, LD(rho), m)
    sc = scale_of(loss, x, sigma, LD(rho), m)
    ok = np.diff(x) < -4 * BAR_PAV * LD(EPS) * sc[1:]
    ends = np.cumsum(seg)
    return np.array([bool(np.all(ok[a:b - 1])) for a, b in zip(ends - seg, ends)])


def prefix_sums_exact(a):
    """every prefix sum of a (multiples of 2^-20) is a float64: checked in integers"""
    k = np.asarray(a, dtype=np.float64) / DYADIC
    if not np.array_equal(k, np.round(k)):
        return False
    acc, worst = 0, 0
    for v in k.astype(np.int64).tolist():
        acc += v
        worst = max(worst, abs(acc))
    return worst < 2 ** 53


# --------------------------------------------------------------------------------------------------- EHRM designs
EHRM_N = 2049
EHRM_B = (-5.0, 0.0, 3.0)
# rho: 2^-14 -> sigma / rho ~ 8 for a middle weight (|prox - m| far above 1e-3: softplus itself);
#      2 -> sigma / rho ~ 2.4e-4 (below 1e-3: the expansion, m = -700 included)
EHRM_RHO = (2.0 ** -14, 2.0)
EHRM_EDGE = [s * x for x in (36.5, 37.5, 700.0, 745.2, 746.0, 1e-300) for s in (1.0, -1.0)] + [0.0]
TH = ((1300, 1340), (1500, 1540))            # positions whose m sits on the threshold of their own sigma_a or sigma_b


def ehrm_weights():
    return weights.get_weights("ehrm", EHRM_N)


def ehrm_thresholds(B, rho):
    sa, sb = ehrm_weights()
    sig = float(sigmoid(B))
    return B + sa * sig / rho, B + sb * sig / rho


def ehrm_design(B, rho, seed=0):
    """sorted m of EHRM_N entries.  The two position ranges of TH hold the thresholds B + sigma_a[i] sigmoid(B) / rho and
    B + sigma_b[i] sigmoid(B) / rho of those very positions, exactly and moved by 1e-12 relative up and down (both weight
    vectors increase over those positions, so the order is kept); the positions between them are spread linearly; below
    position 1100 and from 1700 on: draws within 12 of the thresholds and the edge values on their side"""
    rng = np.random.default_rng([seed, int(B) + 10, int(-math.log2(rho)) + 5])
    ta, tb = ehrm_thresholds(B, rho)
    spans = [(ta, TH[0]), (tb, TH[1])]
    if not ta[TH[0][1] - 1] < tb[TH[1][0]]:                                   # whichever order keeps m sorted
        spans = [(tb, TH[0]), (ta, TH[1])]
    bump = 1.0 + 1e-12 * (np.arange(EHRM_N) % 3 - 1)
    first = spans[0][0][spans[0][1][0]] * (1.0 - 1e-12) - abs(spans[0][0][spans[0][1][0]]) * 1e-9 - 1e-9
    m = np.empty(EHRM_N)
    low = [x for x in EHRM_EDGE if x < first]
    m[:1100] = np.sort(np.concatenate([np.array(low), first - rng.uniform(0.0, 12.0, 1100 - len(low))]))
    lo_i, below = 1100, first
    for t, (i0, i1) in spans:
        vals = t[i0:i1] * bump[i0:i1]
        m[lo_i:i0] = np.linspace(below, vals[0], i0 - lo_i + 2)[1:-1]
        m[i0:i1] = vals
        lo_i, below = i1, vals[-1]
    m[lo_i:1700] = np.linspace(below, below + 1.0, 1700 - lo_i + 1)[1:]
    last = m[1699]
    high = [x for x in EHRM_EDGE if x > last]
    m[1700:] = np.sort(np.concatenate([np.array(high), last + rng.uniform(0.0, 12.0, EHRM_N - 1700 - len(high))]))
    return m


EHRM_MONO_RHO = 1.0


def ehrm_monotone(B):
    """m spread so widely that at EHRM_MONO_RHO neither branch pools anything: the output is the clipped element prox"""
    return np.linspace(-20.0, 20.0, EHRM_N) + B


# A close call: 1700 entries below B with |prox_a - m| between 0.04 and 0.64 (70 % of them below 0.1: the evaluation
# of softplus just beyond the expansion's cut-over at 1e-3), and 349 above it at a distance tuned (by bisection on the reference, to 2^-31) so that f1 is below f2 by
# 5e-9 of their sum: far above what a float64 sum of 2049 terms can be wrong by (1e-13) and what softplus_near claims
# (5e-15), close enough that an expansion used out to |d| = 0.1 (fourth-order term d^4 / 192 at m = 0) turns the branch.
EHRM_CLOSE = dict(B=1.0, rho=2.0 ** -9, t=float.fromhex("0x1.3024249e00000p+1"), n_low=1700)


def ehrm_close_call():
    """-> (B, rho, sorted m)"""
    B, rho, t, k = (EHRM_CLOSE[x] for x in ("B", "rho", "t", "n_low"))
    return B, rho, np.concatenate([np.linspace(B - 1.5, B - 0.5, k), np.linspace(B + t, B + t + 1.0, EHRM_N - k)])


def ehrm_reference(B, rho, m):
    """-> dict(f1, f2, branch, o1, o2): the singleton-stage test in longdouble from longdouble roots"""
    sa, sb = ehrm_weights()
    pa, pb = prox_bce(sa, rho, m), prox_bce(sb, rho, m)
    o1, o2 = np.minimum(pa, LD(B)), np.maximum(pb, LD(B))
    f = lambda s, o: np.sum(ld(s) * softplus(o) + LD(rho) / 2 * (o - ld(m)) ** 2)
    f1, f2 = f(sa, o1), f(sb, o2)
    return dict(f1=f1, f2=f2, branch=0 if f1 <= f2 else 1, pa=pa, pb=pb, o1=o1, o2=o2)
