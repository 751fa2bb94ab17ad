"""csrc/eig.hip restated in NumPy (a helper, not a conftest): the pair schedule (ej_pair), one round of rotations
(k_eig_step), the Rayleigh quotients (k_eig_finish), the sweep loop with its thresholds (launch_eig_jacobi) and the ridge
solve through the basis (launch_ridge_eig), in IEEE fp64.  The m / 2 pairs of a round are disjoint, so a round is one
vectorised update of m rows; the three dot products of a pair are NumPy's pairwise sums where the kernel sums in a block
tree - same thresholds, same order of rotations, another order of additions.  Nothing here calls the library;
tests/test_eig_host.py runs it, tests/test_gpu_eig.py prints its sweep counts beside the device's."""
import numpy as np

SWEEP_CAP = 30
TINY_REL = 1e-13          # tiny = TINY_REL * max diagonal * d
OFF_STOP = 1e-14          # a sweep whose largest |cos| is at most this ends the iteration
ROTATE_MIN = 1e-16        # pairs whose |cos| is not above this are left alone


def round_up(x, m):
    return -(-int(x) // m) * m


def players(d):
    """the even number of players of the circle method: an odd d plays against a dummy, index d"""
    return (int(d) + 1) & ~1


def pairs(m, r):
    """ej_pair for all i = 0 .. m/2 - 1 of round r: (p, q) with p < q, int64 arrays"""
    mm = m - 1
    i = np.arange(m // 2, dtype=np.int64)
    p = (r + i) % mm
    q = (r - i + mm) % mm
    p[0], q[0] = mm, r % mm
    return np.minimum(p, q), np.maximum(p, q)


def step(Bt, Vt, d, m, r, tiny2):
    """k_eig_step for every block of round r, in place.  Returns the largest |cos| the round fed to offmax (0.0 if none)"""
    p, q = pairs(m, r)
    keep = q < d                                   # padding rows / the dummy player of an odd d
    p, q = p[keep], q[keep]
    if p.size == 0:
        return 0.0
    bp, bq = Bt[p], Bt[q]
    a, b, g = np.sum(bp * bp, axis=1), np.sum(bq * bq, axis=1), np.sum(bp * bq, axis=1)
    live = (a > tiny2) & (b > tiny2)               # a null-space row: nothing to orthogonalise against
    if not live.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        cosv = np.where(live, np.abs(g) / np.sqrt(a * b), 0.0)
    off = float(np.max(cosv))
    rot = live & (cosv > ROTATE_MIN)
    if not rot.any():
        return off
    p, q, a, b, g = p[rot], q[rot], a[rot], b[rot], g[rot]
    zeta = (b - a) / (2.0 * g)
    t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    c = 1.0 / np.sqrt(1.0 + t * t)
    s = c * t
    c, s = c[:, None], s[:, None]
    for M in (Bt, Vt):
        x, y = M[p], M[q]
        M[p] = c * x - s * y
        M[q] = s * x + c * y
    return off


def finish(Bt, Vt, d):
    """k_eig_finish: lambda_j = row j of Vt . row j of Bt, clamped at 0 and 0 on the padding; V = Vt^T"""
    lam = np.sum(Vt * Bt, axis=1)
    lam = np.where((np.arange(lam.size) < d) & (lam > 0.0), lam, 0.0)
    return lam, np.ascontiguousarray(Vt.T)


def jacobi(G, sweep_cap=SWEEP_CAP, trace=None):
    """launch_eig_jacobi on G (d x d), padded to ld = round_up(d, 4).  Returns dict(Vt, V, lam, ld, sweeps); sweeps == 0:
    not converged within the cap (V and lam are None, Vt the last iterate).  trace: a list that receives the largest
    |cos| of every sweep."""
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[0]
    ld = round_up(d, 4)
    Bt = np.zeros((ld, ld))
    Bt[:d, :d] = G
    Vt = np.eye(ld)
    m = players(d)
    if m < 2:
        raise ValueError("d >= 1 is needed")       # (d = 1 has m = 2: its one pair meets the dummy and is skipped)
    dmax = max(0.0, float(np.max(np.diag(G))))
    tiny = TINY_REL * dmax * float(d)
    tiny2 = tiny * tiny
    for sweep in range(1, sweep_cap + 1):
        off = 0.0
        for r in range(m - 1):
            off = max(off, step(Bt, Vt, d, m, r, tiny2))
        if trace is not None:
            trace.append(off)
        if off <= OFF_STOP:
            lam, V = finish(Bt, Vt, d)
            return dict(Vt=Vt, V=V, lam=lam, ld=ld, sweeps=sweep)
    return dict(Vt=Vt, V=None, lam=None, ld=ld, sweeps=0)


NULL_CUT = 1e-13          # reg == 0: rows with lambda <= NULL_CUT * ld * max lambda get the coefficient 0


def coef(Vt, x, lam, rho, reg, guard):
    """k_eig_coef.  guard False: the plain quotient as first shipped (0 / 0 = NaN where rho lambda + reg is 0); True:
    with reg == 0 the rows of the null space (lambda at most NULL_CUT ld max lambda, the padding among them) get the
    coefficient 0"""
    num = Vt @ x
    den = rho * lam + reg
    if not guard:
        with np.errstate(divide="ignore", invalid="ignore"):
            return num / den
    cut = NULL_CUT * lam.size * float(np.max(lam)) if reg == 0.0 else -1.0
    solve = lam > cut
    return np.divide(num, den, out=np.zeros_like(num), where=solve)


REFINEMENTS = 2           # EJ_REFINE of eig.hip


def ridge(G_ld, dec, q_ld, rho, reg, refinements=REFINEMENTS, guard=True):
    """launch_ridge_eig: (rho G + reg I) w = rho q through the decomposition, then `refinements` steps of iterative
    refinement against G itself.  All arrays have the padded length ld."""
    Vt, V, lam = dec["Vt"], dec["V"], dec["lam"]
    w = V @ coef(Vt, rho * q_ld, lam, rho, reg, guard)
    for _ in range(refinements):
        res = rho * q_ld - (rho * (G_ld @ w) + reg * w)
        w = w + V @ coef(Vt, res, lam, rho, reg, guard)
    return w


def pad(G, q=None):
    d = G.shape[0]
    ld = round_up(d, 4)
    Gp = np.zeros((ld, ld))
    Gp[:d, :d] = G
    if q is None:
        return Gp
    qp = np.zeros(ld)
    qp[:d] = q
    return Gp, qp


# ---------------------------------------------------------------------------------------- measures (longdouble)
def orthogonality(Vt):
    """max |Vt Vt^T - I| (in longdouble)"""
    V = Vt.astype(np.longdouble)
    return float(np.max(np.abs(V @ V.T - np.eye(V.shape[0], dtype=np.longdouble))))


def eigen_residual(mat, Vt, lam):
    """max_j ||G v_j - lambda_j v_j||_2 over the d columns of the problem, G v_j through Mat.mv in longdouble"""
    d = mat.d
    worst = 0.0
    for j in range(d):
        v = Vt[j, :d].astype(np.longdouble)
        r = mat.mv(v) - np.longdouble(lam[j]) * v
        worst = max(worst, float(np.sqrt(np.sum(r * r))))
    return worst
