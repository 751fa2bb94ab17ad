"""Matrices, planted minimisers, bounds and the instance table for the d-space w-steps (csrc/wstep.hip, csrc/lasso_fs.hip)
run through rbl_k_wstep_seq (a helper, not a conftest).  Nothing here calls the library; tests/test_wstep_host.py checks
this file on the CPU, tests/test_gpu_wstep.py uses it against the kernels.  The fixtures, widths and the two bounds of the
eigendecomposition ridge (csrc/eig.hip, route 2 of the entry) are in the section of that name; tests/test_eig_host.py
checks them and tests/test_gpu_eig.py uses them.

Instance table.  A persistent w-step launches ceil(ld / WP_RPB) blocks of WP_THREADS threads.  A block keeps ld + 48
doubles (the vector, 16 block sums, WP_RPB + 16 for its rows of the product) and, when they fit the LDS budget beside
that, its WP_RPB rows of G: 8 (ld + 48) + 8 * 16 * ld <= 156 KB, ld <= 1171.8, so ld <= 1168 in multiples of 4.  A thread owns 4
vector elements up to ld = 4 * WP_THREADS = 1024 and 8 above; beyond WSTEP_PERSIST_MAX_LD = 8 * WP_THREADS the batched
launches run.  INSTANCES holds the outcome as data; instance_from_constants() is the derivation the host test holds
it against, the GPU tests hold the report of every launch against INSTANCES.

Matrices.  G = diag(s) + U U^T with U (d x 8) in multiples of 2^-3 times a power of two and s in multiples of 2^-30:
every entry of G is exact in fp64, so lambda_min(G) >= min s and ||G||_2 <= max s + ||U||_F^2 hold for the matrix the
device sees, without an eigensolver.  Three kinds: "well" (s in [1, 64]), "ill" (6 distinct values of s, log-spaced
from 2^-20 to 64: with the rank-8 term some 50 eigenvalue clusters over 8 decades - the CG needs 170-300 iterations at
any width, where a spectrum without clusters needs more than the persistent kernel's 4000) and collinear() (D^T D of a thin integer D with
two exactly collinear columns; PSD, singular).

Planted minimisers.  w* is chosen and q formed from it in np.longdouble, then rounded ONCE to fp64:
    ridge  q = (G + (reg / rho) I + diag(l2) / rho) w*
    lasso  q = G w* + kappa o s,  s_j = sign(w*_j) on the support, |s_j| <= 0.9 off it
    Huber  q = G w* + h_t'(w*) / rho, coordinates on both sides of t, two of them within 1e-3 t of it
The rounding of q moves the minimiser by at most eps ||q||_2 / lambda_min; the bounds below carry that term.

Bounds (eps = 2^-52).  A = rho G + reg I + diag(l2), ||A||_2 <= rho (max s + ||U||_F^2) + reg + max l2 = A_hi,
lambda_min(A) >= rho min s + reg + min l2 = A_lo.
    ridge   the CG stops on the recurrence residual, ||r_k||_2 <= tol ||rho q||_2; the true residual
            rho (G w - q) + reg w + l2 o w is allowed  tol ||rho q||_2 + iters 4 eps A_hi ||w||_2  (iters as reported: the
            textbook drift of the recurrence residual), and ||w - w*||_2 that over A_lo (+ the rounding of q)
    Huber   the nonlinear CG stops on max_j |g_j| <= tol max(max rho |q|, reg / 2) with G w kept by recurrence:
            max_j |g_j| of the true gradient is allowed  tol max(max rho |q|, reg / 2) + iters 4 eps A_hi ||w||_2  with
            A_hi = rho ||G||_2 + reg / (2 t), and ||w - w*||_2 sqrt(d) times that over rho min s (strong convexity)
    lasso   the active-set kernel ends when the active coordinates satisfy |g_a + kappa_a sign(w_a)| <= 1e-12 scale and
            the others |g_i| <= kappa_i (1 + 1e-12) + 1e-14 scale, scale = max(||q||_inf, max kappa), on gradients it
            sums over the nnz active columns: the KKT residual is allowed  2.01e-12 scale + 2 (nnz + 2) eps max_j (|G| |w| +
            |q|)_j, and ||w - w*||_2 sqrt(d) times that over min s.  FISTA's stop rule (the last step's length) bounds no
            KKT residual a priori: a w-step that fell back is held to 1e-10 scale, the constant of the suite's w-step
            tests, which also caps every bound above.
"""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52

# ------------------------------------------------------------------------------------------------ the instance table
WP_RPB, WP_THREADS, LDS_BUDGET, WSTEP_PERSIST_MAX_LD = 16, 256, 156 * 1024, 2048
# (ld_lo, ld_hi, glds, per): ld in multiples of 4
INSTANCES = [(4, 1024, 1, 4), (1028, 1168, 1, 8), (1172, 2048, 0, 8)]
# ld of every edge the GPU tests run (d = ld except where the padding is the point)
WIDTHS = [4, 16, 20, 64, 68, 252, 512, 516, 1024, 1028, 1100, 1168, 1172, 1536, 1540, 2048, 2052]
PERSIST_D = [1, 3] + [w for w in WIDTHS[1:] if w <= WSTEP_PERSIST_MAX_LD]        # d = 1 and d = 3 are ld = 4
BATCHED_ROUTE1_D = [1, 3, 20, 1024, 1028, 2048]
BATCHED_NATURAL_D = [2052, 4100]


def round_up(x, m):
    return -(-int(x) // m) * m


def instance(ld):
    """dict(glds, per, nblocks, lds_bytes) of the persistent launch at row stride ld, None where the batched route runs"""
    for lo, hi, glds, per in INSTANCES:
        if lo <= ld <= hi:
            fixed = 8 * (ld + 16 + WP_RPB + 16)
            return dict(glds=glds, per=per, nblocks=-(-ld // WP_RPB), lds_bytes=fixed + (8 * WP_RPB * ld if glds else 0))
    return None


def instance_from_constants(ld):
    """the same from the four constants alone (the host test compares every multiple of 4 with instance())"""
    if ld < 4 or ld > WSTEP_PERSIST_MAX_LD:
        return None
    fixed = 8 * (ld + 16 + WP_RPB + 16)
    rows = 8 * WP_RPB * ld
    glds = 1 if fixed + rows <= LDS_BUDGET else 0
    per = 4 if ld <= 4 * WP_THREADS else 8
    assert per * WP_THREADS >= ld
    return dict(glds=glds, per=per, nblocks=(ld + WP_RPB - 1) // WP_RPB, lds_bytes=fixed + (rows if glds else 0))


# ------------------------------------------------------------------------------------------------------- matrices
class Mat:
    """G (d x d, fp64) = diag(s) + B^T B EXACTLY (B: k x d), with lam_lo <= lambda_min(G), ||G||_2 <= lam_hi"""

    def __init__(self, G, s, B, lam_lo, lam_hi, kind):
        self.G, self.lam_lo, self.lam_hi, self.kind, self.d = G, float(lam_lo), float(lam_hi), kind, G.shape[0]
        self._s, self._B = s.astype(LD), B.astype(LD)

    def mv(self, w):
        """G w in longdouble, through the factors (matrix() and collinear() assert that G is exactly their product)"""
        wl = np.asarray(w).astype(LD)
        return self._s * wl + self._B.T @ (self._B @ wl)


_mats = {}


def matrix(d, kind):
    """kind "well" or "ill"; cached (the tests share them and leave them unchanged)"""
    key = (d, kind)
    if key in _mats:
        return _mats[key]
    rng = np.random.default_rng([d, 17, kind == "ill"])
    scale = 2.0 ** -max(0, round(math.log2(max(d, 4)) / 2) - 1)          # ||U||_F^2 stays of order 10 - 100
    U = rng.integers(-8, 9, size=(d, 8)).astype(np.float64) / 8.0 * scale
    if kind == "well":
        s = 1.0 + rng.integers(0, 63 * 2 ** 10 + 1, size=d) / 2.0 ** 10
    else:
        levels = np.round(2.0 ** np.linspace(-20.0, 6.0, 6) * 2.0 ** 30) / 2.0 ** 30
        s = levels[rng.integers(0, 6, size=d)]
        s[rng.integers(0, d)] = levels[0]
    G = U @ U.T
    G[np.diag_indices(d)] += s
    # exactness: U's products are multiples of 2^-6 scale^2 below 2^7, s of 2^-30 - all within 53 bits
    UL = U.astype(LD)
    for i in range(0, d, 256):
        blk = UL[i:i + 256] @ UL.T
        blk[np.arange(blk.shape[0]), i + np.arange(blk.shape[0])] += s[i:i + 256].astype(LD)
        assert np.array_equal(G[i:i + 256].astype(LD), blk)
    m = Mat(G, s, U.T, s.min(), s.max() + float(np.sum(UL ** 2)) * (1 + 1e-12), kind)
    _mats[key] = m
    return m


def collinear(d, n=None):
    """G = D^T D (exact integers) of a thin D (n = d + 32 rows) whose column 5 is 2 col 3 - col 4 (d >= 8), as the
    generator's redundant columns give: PSD, singular, no lower bound"""
    n = d + 32 if n is None else n
    rng = np.random.default_rng([d, 23])
    D = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    D[:, 5] = 2.0 * D[:, 3] - D[:, 4]
    G = D.T @ D                                                     # integers below 2^53: exact in any order
    assert np.array_equal(G, (D.astype(np.int64).T @ D.astype(np.int64)).astype(np.float64))
    return Mat(G, np.zeros(d), D, 0.0, float(np.sum(D * D)), "collinear"), D


# ------------------------------------------------------------- the eigendecomposition ridge (csrc/eig.hip), route 2
# Widths: the smallest at which each loop shape of eig.hip changes.  1: one player and the dummy, nothing rotates; 2, 3: 3 is
# odd (a dummy player) with ld = 4; 5: padded past one packet (ld = 8); 63, 64, 65: the 64-lane stride of k_eig_coef /
# k_eig_apply; 255, 256, 257, 260: one trip against two of the EJ_THREADS = 256 loops, with ld = d and ld > d.
EIG_WIDTHS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 260]
EIG_EXACT = ["identity", "diagzero", "zero", "rankone"]
EIG_ILL_D = [3, 5, 24, 63, 64, 65, 132]          # "ill" where the Jacobi converges within its 30 sweeps ...
EIG_ILL_STALLS_D = 257                           # ... and where the restatement does not
EIG_COLLINEAR_D = [w for w in EIG_WIDTHS if w >= 8]
EIG_WIDE_D = [1000, 2048]                        # "well" only: the benchmark's width and the limit of the route
EIG_MAX_LD = 2048                                # rbl_gram_finish decomposes up to here; beyond, the CG runs
EIG_BEYOND_D = 2052
# every decomposition the GPU tests run and tests/test_eig_host.py restates (the two wide ones are restated once, by hand:
# EIG_REF_WIDE below)
EIG_CASES = ([("well", d) for d in EIG_WIDTHS] + [("ill", d) for d in EIG_ILL_D] + [("collinear", d) for d in EIG_COLLINEAR_D]
             + [(k, d) for k in EIG_EXACT for d in EIG_WIDTHS])
# ridge through the basis: planted minimisers on these, at the four (rho, reg) of eig_rho_reg(d)
EIG_RIDGE_CASES = [c for c in EIG_CASES if c[0] in ("well", "ill", "collinear")]


def eig_rho_reg(d):
    """(rho, reg): the w-step tests' own pair, a small rho, and the cap of the rho schedule (217 d) with reg = 0.01 and
    with the reference default 1e-4"""
    return [(1.0, 0.5), (2.0 ** -12, 0.5), (217.0 * d, 0.01), (217.0 * d, 1e-4)]


def eig_matrix(kind, d):
    """the Mat of an EIG_CASES entry.  The exact kinds: "identity" 3 I; "diagzero" diag(1 + j mod 7) with entry d // 2
    zero (a null row before any rotation); "zero"; "rankone" u u^T with integer u, every third entry zero (null rows from
    the start) - all exact in fp64, mv through the factors in longdouble as for the others."""
    if kind in ("well", "ill"):
        return matrix(d, kind)
    if kind == "collinear":
        return collinear(d)[0]
    j = np.arange(d)
    none = np.zeros((1, d))
    if kind == "identity":
        return Mat(3.0 * np.eye(d), np.full(d, 3.0), none, 3.0, 3.0, kind)
    if kind == "diagzero":
        s = 1.0 + j % 7
        s[d // 2] = 0.0
        return Mat(np.diag(s), s, none, 0.0, float(np.max(s)), kind)
    if kind == "zero":
        return Mat(np.zeros((d, d)), np.zeros(d), none, 0.0, 0.0, kind)
    if kind == "rankone":
        u = np.where(j % 3 == 2, 0.0, (j % 5 + 1.0) * np.where(j % 2, -1.0, 1.0))
        return Mat(np.outer(u, u), np.zeros(d), u[None, :], 0.0, float(u @ u), kind)
    raise ValueError(kind)


def eig_null_rows(kind, d):
    """rows of G that are zero from the start: the Jacobi must leave them (and their columns of V) alone"""
    j = np.arange(d)
    return {"diagzero": j[j == d // 2], "zero": j, "rankone": j[j % 3 == 2]}.get(kind, j[:0])


# The two bounds the project did not have, both K d eps:
#   EIG_ORTH_K   max |Vt Vt^T - I| <= EIG_ORTH_K d eps
#   EIG_RES_K    max_j ||G v_j - lambda_j v_j||_2 <= EIG_RES_K d eps lam_hi   (and |lambda - eigvalsh| the same)
# K = 4 x the largest value the NumPy restatement (tests/eig_ref.py) reaches over EIG_CASES and EIG_REF_WIDE; the device
# sums a row in a block tree where NumPy sums pairwise, 4 covers the order.  Restatement, in units of d eps:
#   orthogonality   largest 3.01 (ill, d = 132); ill 0.46 - 3.01, collinear 1.17 - 1.59, well 0.15 - 1.10, rank one <= 0.21
#   residual        largest 31.3 (collinear, d = 63: a null vector is only as good as the threshold that leaves its row
#                   alone, 1e-13 d max diag); collinear 1.4 - 31.3, ill 0.12 - 2.71, well 0.19 - 0.80, rank one <= 0.23
# (tests/test_eig_host.py prints the table, holds every case to half its bound and the constants to 4 x the largest)
EIG_ORTH_K = 12.1
EIG_RES_K = 126.0
# the restatement on the wide matrices (minutes on a CPU, so run once and kept as data; measured on 64 sampled rows):
# d -> (sweeps, orthogonality and residual in units of d eps)
EIG_REF_WIDE = {1000: (6, 1.10, 0.77), 2048: (6, 1.15, 0.89)}
# sweeps the restatement needs per fixture (the host test allows its live count one either way); the GPU tests print
# them beside the device's and assert no equality
EIG_REF_SWEEPS = {("well", 1): 1, ("well", 2): 2, ("well", 3): 4, ("well", 5): 4, ("well", 63): 5, ("well", 64): 6,
                  ("well", 65): 6, ("well", 255): 6, ("well", 256): 6, ("well", 257): 6, ("well", 260): 6,
                  ("well", 1000): 6, ("well", 2048): 6,
                  ("ill", 3): 4, ("ill", 5): 5, ("ill", 24): 10, ("ill", 63): 18, ("ill", 64): 19, ("ill", 65): 18,
                  ("ill", 132): 27,
                  ("collinear", 63): 11, ("collinear", 64): 11, ("collinear", 65): 11, ("collinear", 255): 15,
                  ("collinear", 256): 15, ("collinear", 257): 16, ("collinear", 260): 15}
EIG_REF_SWEEPS.update({("identity", d): 1 for d in EIG_WIDTHS})
EIG_REF_SWEEPS.update({("diagzero", d): 1 for d in EIG_WIDTHS})
EIG_REF_SWEEPS.update({("zero", d): 1 for d in EIG_WIDTHS})
EIG_REF_SWEEPS.update({("rankone", d): (1 if d == 1 else 2) for d in EIG_WIDTHS})


def drifting_rhs_in_range(m, q0, K=3, seed=0):
    """K right-hand sides that drift inside range(G): q_k = q_{k-1} + 1e-3 x (G u_k scaled to unit RMS), rounded to fp64.
    This is all a solver's right-hand side can do - q = D^T c lies in range(D^T) = range(G) - and on a singular G it is
    what keeps the problem the solver's: a component of q in the null space is divided by reg alone, ||w|| = rho 1e-3 /
    reg (1e5 - 1e6 at the rho cap with reg = 1e-4, which no iterate has), and with reg = 0 the system has no solution."""
    rng = np.random.default_rng([m.d, 67, seed])
    Q = np.empty((K, m.d))
    q = np.array(q0, dtype=np.float64)
    for k in range(K):
        if k:
            t = np.asarray(m.mv(rng.standard_normal(m.d)), dtype=np.float64)
            q = q + 1e-3 * t / float(np.sqrt(np.mean(t * t)))
        Q[k] = q
    return Q


def eig_drift(m, q0, K=3):
    """the drifting right-hand sides of the route 2 tests: drifting_rhs without jumps where G is non-singular (any
    direction is in range), drifting_rhs_in_range where it is singular"""
    return drifting_rhs(q0, K=K, jumps=()) if m.lam_lo > 0 else drifting_rhs_in_range(m, q0, K)


def eig_orth_bound(d):
    return EIG_ORTH_K * d * EPS


def eig_res_bound(m):
    return EIG_RES_K * m.d * EPS * m.lam_hi


# ---------------------------------------------------------------------------------------------- planted minimisers
def hub_g(w, reg, t):
    w = np.asarray(w)
    return np.where(np.abs(w) <= t, reg * w / (2 * t), 0.5 * reg * np.sign(w))


def plant_ridge(m, rho, reg, l2=None, seed=0):
    rng = np.random.default_rng([m.d, 31, seed])
    w = rng.standard_normal(m.d)
    wl = w.astype(LD)
    q = m.mv(wl) + (LD(reg) / LD(rho)) * wl
    if l2 is not None:
        q = q + (np.asarray(l2).astype(LD) / LD(rho)) * wl
    return w, np.asarray(q, dtype=np.float64)


def plant_huber(m, rho, reg, t, seed=0):
    rng = np.random.default_rng([m.d, 37, seed])
    d = m.d
    w = np.where(rng.random(d) < 0.5, 0.6 * t, 3.0 * t) * rng.standard_normal(d)      # both sides of t
    w[0] = t * (1 - 5e-4)                                                              # within 1e-3 t, inside
    if d > 1:
        w[d - 1] = -t * (1 + 5e-4)                                                     # and outside
    wl = w.astype(LD)
    hg = np.where(np.abs(wl) <= LD(t), LD(reg) * wl / (2 * LD(t)), LD(0.5) * LD(reg) * np.sign(wl))
    q = m.mv(wl) + hg / LD(rho)
    return w, np.asarray(q, dtype=np.float64)


def plant_lasso(m, kappa, nnz, seed=0, shift=None):
    """kappa: scalar or (d,) thresholds; shift: (d,) added to the diagonal of G (l2 / rho).  Returns (w*, q, s)"""
    rng = np.random.default_rng([m.d, 41, seed, nnz])
    d = m.d
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (d,))
    sup = rng.choice(d, size=nnz, replace=False)
    w = np.zeros(d)
    w[sup] = rng.choice([-1.0, 1.0], size=nnz) * (0.5 + rng.random(nnz))
    s = 0.9 * (2.0 * rng.random(d) - 1.0)
    s[sup] = np.sign(w[sup])
    q = m.mv(w) + kap.astype(LD) * s.astype(LD)
    if shift is not None:
        q = q + np.asarray(shift).astype(LD) * w.astype(LD)
    return w, np.asarray(q, dtype=np.float64), s


# ------------------------------------------------------------------------------------------------ residuals (longdouble)
def ridge_residual(m, q, rho, reg, w, l2=None):
    wl = np.asarray(w).astype(LD)
    r = LD(rho) * (m.mv(wl) - np.asarray(q).astype(LD)) + LD(reg) * wl
    if l2 is not None:
        r = r + np.asarray(l2).astype(LD) * wl
    return r


def huber_gradient(m, q, rho, reg, t, w):
    wl = np.asarray(w).astype(LD)
    hg = np.where(np.abs(wl) <= LD(t), LD(reg) * wl / (2 * LD(t)), LD(0.5) * LD(reg) * np.sign(wl))
    return LD(rho) * (m.mv(wl) - np.asarray(q).astype(LD)) + hg


def huber_objective(m, q, rho, reg, t, w):
    wl = np.asarray(w).astype(LD)
    h = np.where(np.abs(wl) <= LD(t), LD(reg) * wl * wl / (4 * LD(t)), LD(0.5) * LD(reg) * (np.abs(wl) - LD(t) / 2))
    return float(LD(rho) * (LD(0.5) * wl @ m.mv(wl) - np.asarray(q).astype(LD) @ wl) + np.sum(h))


def lasso_kkt(m, q, kappa, w, shift=None):
    """max_j of |g_j + kappa_j sign(w_j)| (w_j != 0) and max(|g_j| - kappa_j, 0) (w_j = 0), g = (G + diag(shift)) w - q"""
    wl = np.asarray(w).astype(LD)
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), wl.shape).astype(LD)
    g = m.mv(wl) - np.asarray(q).astype(LD)
    if shift is not None:
        g = g + np.asarray(shift).astype(LD) * wl
    on = wl != 0
    r = np.where(on, np.abs(g + kap * np.sign(wl)), np.maximum(np.abs(g) - kap, 0))
    return float(np.max(r))


def lasso_objective(m, q, kappa, w, shift=None):
    wl = np.asarray(w).astype(LD)
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), wl.shape).astype(LD)
    f = LD(0.5) * wl @ m.mv(wl) - np.asarray(q).astype(LD) @ wl + np.sum(kap * np.abs(wl))
    if shift is not None:
        f = f + LD(0.5) * np.sum(np.asarray(shift).astype(LD) * wl * wl)
    return float(f)


def absGw(m, w):
    return np.abs(m.G) @ np.abs(np.asarray(w, dtype=np.float64))


# --------------------------------------------------------------------------------------------------------- bounds
SUITE = 1e-10          # x scale: the constant of the existing w-step tests; no bound here is looser


def a_hi(m, rho, reg, l2=None):
    return rho * m.lam_hi + reg + (float(np.max(l2)) if l2 is not None else 0.0)


def a_lo(m, rho, reg, l2=None):
    return rho * m.lam_lo + reg + (float(np.min(l2)) if l2 is not None else 0.0)


def ridge_bound(m, q, rho, reg, tol, iters, w, l2=None):
    """on ||true residual||_2"""
    nq = float(np.linalg.norm(rho * np.asarray(q, dtype=np.float64)))
    b = tol * nq + iters * 4 * EPS * a_hi(m, rho, reg, l2) * float(np.linalg.norm(w))
    return min(b, SUITE * nq)


def ridge_w_bound(m, q, rho, reg, tol, iters, w, l2=None):
    """on ||w - w*||_2: the residual bound and the rounding of q (rho eps ||q||_2), over lambda_min(A)"""
    nq = float(np.linalg.norm(rho * np.asarray(q, dtype=np.float64)))
    return (ridge_bound(m, q, rho, reg, tol, iters, w, l2) + EPS * nq) / a_lo(m, rho, reg, l2)


def huber_scale(q, rho, reg):
    return max(float(np.max(np.abs(rho * np.asarray(q)))), 0.5 * reg)


def huber_bound(m, q, rho, reg, t, tol, iters, w):
    """on max_j |true gradient_j|"""
    sc = huber_scale(q, rho, reg)
    b = tol * sc + iters * 4 * EPS * (rho * m.lam_hi + reg / (2 * t)) * float(np.linalg.norm(w))
    return min(b, SUITE * sc)


def huber_w_bound(m, q, rho, reg, t, tol, iters, w):
    nq = float(np.linalg.norm(rho * np.asarray(q, dtype=np.float64)))
    return (math.sqrt(m.d) * huber_bound(m, q, rho, reg, t, tol, iters, w) + EPS * nq) / (rho * m.lam_lo)


def lasso_scale(q, kappa):
    return max(float(np.max(np.abs(q))), float(np.max(kappa)))


def lasso_bound(m, q, kappa, w, fell_back):
    """on the KKT residual"""
    sc = lasso_scale(q, kappa)
    if fell_back:
        return SUITE * sc
    nnz = int(np.count_nonzero(w))
    b = 2.01e-12 * sc + 2 * (nnz + 2) * EPS * float(np.max(absGw(m, w) + np.abs(q)))
    return min(b, SUITE * sc)


def lasso_w_bound(m, q, kappa, w, fell_back, lam_lo=None):
    lo = m.lam_lo if lam_lo is None else lam_lo
    return (math.sqrt(m.d) * lasso_bound(m, q, kappa, w, fell_back) + EPS * float(np.linalg.norm(q))) / lo


# --------------------------------------------------------------------------------------------- exact integer fixtures
def _next_prime(n):
    def is_p(k):
        if k % 2 == 0:
            return k == 2
        for f in range(3, int(math.isqrt(k)) + 1, 2):
            if k % f == 0:
                return False
        return True
    n += 1
    while not is_p(n):
        n += 1
    return n


_ints = {}


def integer_fixture(d):
    """G (d x d int64, dense, NOT symmetric: every entry different modulo the prime p > d^2 - the kernels read G by rows,
    and with no CG iteration nothing needs symmetry) and w0 (int64, 1 <= |w0_j| <= 3).  Every product and partial sum
    is an integer below 2^53, so any order of summation gives the same bits."""
    if d in _ints:
        return _ints[d]
    p = _next_prime(max(d * d, 16))
    mult = 7919 if p != 7919 else 104729
    idx = (np.arange(d, dtype=np.int64)[:, None] * d + np.arange(d, dtype=np.int64)[None, :])
    G = (idx * mult) % p - p // 2
    rng = np.random.default_rng([d, 43])
    w0 = rng.integers(1, 4, size=d) * rng.choice([-1, 1], size=d)
    assert d * (p // 2 + 4) * 3 < 2 ** 53
    _ints[d] = (G, w0.astype(np.int64), p)
    return _ints[d]


def integer_ridge(d, l2=False):
    """rho = 1, reg = 1 (with l2: integer penalties 1..5 in the place of reg): (G + I) w0 = q exactly, the CG's first
    residual is exactly zero.  Returns G, w0, q (float64, exact), Gw (int64), l2 or None"""
    G, w0, _ = integer_fixture(d)
    pen = (np.arange(d, dtype=np.int64) % 5 + 1) if l2 else np.ones(d, dtype=np.int64)
    Gw = G @ w0
    q = Gw + pen * w0
    return G.astype(np.float64), w0.astype(np.float64), q.astype(np.float64), Gw, (pen.astype(np.float64) if l2 else None)


def integer_huber(d):
    """rho = 1, reg = 1, t = 1/2 < |w0_j|: the Huber gradient is +- 1/2, q = G w0 + sign(w0) / 2 is exact and the first
    gradient exactly zero"""
    G, w0, _ = integer_fixture(d)
    Gw = G @ w0
    q = Gw.astype(np.float64) + 0.5 * np.sign(w0)
    return G.astype(np.float64), w0.astype(np.float64), q, Gw


# ------------------------------------------------------------------------------------------- NumPy restatements
def cg_numpy(G, q, rho, reg, tol, w0, l2=None, max_iter=20000):
    """Textbook CG on (rho G + reg I + diag(l2)) w = rho q from w0, stopped as the kernels stop: r'r <= tol^2 b'b on the
    recurrence residual (or a step of length 0).  Returns (w, iterations, the recurrence residual).  Plain float64 NumPy:
    not the code under test."""
    A = lambda x: rho * (G @ x) + reg * x + (l2 * x if l2 is not None else 0.0)
    w = np.array(w0, dtype=np.float64)
    b = rho * np.asarray(q, dtype=np.float64)
    r = b - A(w)
    p = r.copy()
    rr, thr = r @ r, tol * tol * (b @ b)
    it = 0
    while rr > thr and it < max_iter:
        Ap = A(p)
        pAp = p @ Ap
        alpha = rr / pAp if pAp > 0 else 0.0
        w += alpha * p
        r -= alpha * Ap
        rn = r @ r
        p = r + (rn / rr) * p
        rr = rn
        it += 1
        if alpha == 0.0:
            break
    return w, it, r


# ------------------------------------------------------------------------------------------------------ sequences
# reg = 48 beside s in [1, 64]: the CG gains about 0.7 digits per iteration, so a drift step (8 digits) ends after about
# 10 - 12 iterations and a jump (11 digits) after 14 - 17, also at d = 20 where it would otherwise end by finite termination
SEQ_D, SEQ_RHO, SEQ_REG, SEQ_JUMPS = [20, 1028, 2048], 1.0, 48.0, (4, 8)


def drifting_rhs(q0, K=12, jumps=SEQ_JUMPS, seed=0):
    """K right-hand sides: q_k = q_{k-1} + 1e-3 x a unit-scale direction, and a step of order 1 at the jumps"""
    rng = np.random.default_rng([q0.size, 47, seed])
    Q = np.empty((K, q0.size))
    q = np.array(q0, dtype=np.float64)
    for k in range(K):
        if k:
            q = q + (1.0 if k in jumps else 1e-3) * rng.standard_normal(q0.size)
        Q[k] = q
    return Q
