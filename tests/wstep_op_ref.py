"""NumPy / SciPy restatement of the operator w-step (csrc/wstep_op.hip: a handle created with RBL_CREATE_NO_GRAM) and
an ADMM loop around exact w-steps that never forms the d x d Gram matrix.  A helper, not a conftest: nothing in the
package imports it.

    A p = rho D^T (D p) + reg p + l2 .* p           (the operator; D sparse, n x d)
    ridge:        A w = rho q                        warm-started CG, stop r'r <= tol^2 ||rho q||^2 or alpha == 0
    elastic net:  min 1/2 w'(D^T D + diag(l2)/rho) w - q'w + sum_j kappa_j |w_j|,  kappa_j = l1_j / (2 rho)
                  FISTA with gradient restart, step 1/L, stop max|dw| <= tol max(1, max|w|)

For wide shapes (n < d) the exact ridge solve goes through the n x n identity
    (rho D^T D + B)^-1 = B^-1 - B^-1 D^T (I/rho + D B^-1 D^T)^-1 D B^-1,       B = diag(b) > 0,
with the coordinates where b_j = 0 (an unpenalised intercept) eliminated by a Schur complement."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import admm as _admm
from oracle import objective as _obj
from oracle import weights as _w

CHUNK = 2048          # wstep_op_plan.h: OP_CHUNK, the reduction's chunk
GRAM_MAX_LD = 16384   # the Gram route's widest ld


def op_apply(D, p, rho, reg=0.0, l2=None):
    """A p = rho D^T (D p) + reg p (l2 is None) or + l2 .* p"""
    y = rho * (D.T @ (D @ p))
    return y + (reg * p if l2 is None else l2 * p)


def power_L(D, iters=100):
    """L = 1.02 lambda as rbl_gram_finish takes it: `iters` power steps from the library's fixed start vector"""
    d = D.shape[1]
    j = np.arange(1, d + 1, dtype=np.uint64)
    h = j * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    x = 0.5 + (h & np.uint64(0xffff)).astype(np.float64) / 65536.0
    x /= np.linalg.norm(x)
    lam = 0.0
    for _ in range(iters):
        y = D.T @ (D @ x)
        lam = float(np.linalg.norm(y))
        x = y / lam if lam > 0 else y
    L = 1.02 * lam
    return L if L > 0 else 1.0


def cg(D, q, rho, reg=0.0, l2=None, w0=None, tol=1e-13, max_iter=100000):
    """k_cg_init / k_cg_update on the operator -> (w, iterations, converged)"""
    d = D.shape[1]
    w = np.zeros(d) if w0 is None else np.array(w0, dtype=np.float64)
    b = rho * q
    r = b - op_apply(D, w, rho, reg, l2)
    p = r.copy()
    rr, thr = float(r @ r), tol * tol * float(b @ b)
    if rr <= thr:
        return w, 0, True
    for it in range(1, max_iter + 1):
        Ap = op_apply(D, p, rho, reg, l2)
        pAp = float(p @ Ap)
        alpha = rr / pAp if pAp > 0 else 0.0
        w = w + alpha * p
        r = r - alpha * Ap
        rr_new = float(r @ r)
        beta = rr_new / rr if rr > 0 else 0.0
        p = r + beta * p
        rr = rr_new
        if rr <= thr or alpha == 0.0:
            return w, it, True
    return w, max_iter, False


def fista(D, q, rho, reg=0.0, l1=None, l2=None, L=None, w0=None, tol=1e-13, max_iter=100000):
    """k_fista_update<PEN> on the operator -> (w, iterations, converged).  Scalar form (l1 is None): kappa = reg/(2 rho)."""
    d = D.shape[1]
    w = np.zeros(d) if w0 is None else np.array(w0, dtype=np.float64)
    L = power_L(D) if L is None else L
    if l1 is not None or l2 is not None:
        l1 = np.zeros(d) if l1 is None else np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,))
        l2 = np.zeros(d) if l2 is None else np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,))
        L = L + float(np.max(l2)) / rho
        kap, dg = l1 / (2.0 * rho) / L, l2 / rho
    else:
        kap, dg = reg / (2.0 * rho) / L, 0.0
    yk, t = w.copy(), 1.0
    for it in range(1, max_iter + 1):
        b = yk - (D.T @ (D @ yk) + dg * yk - q) / L
        x = np.sign(b) * np.maximum(np.abs(b) - kap, 0.0)
        dw = x - w
        restart = float((yk - x) @ dw) > 0.0
        tn = 1.0 if restart else 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        coef = 0.0 if restart else (t - 1.0) / tn
        w, yk, t = x, x + coef * dw, tn
        if float(np.max(np.abs(dw))) <= tol * max(1.0, float(np.max(np.abs(w)))):
            return w, it, True
    return w, max_iter, False


def ridge_residual(D, q, rho, reg, l2, w):
    """||A w - rho q||_2 / ||rho q||_2 in float64 from the sparse matrix"""
    b = rho * q
    return float(np.linalg.norm(op_apply(D, w, rho, reg, l2) - b) / np.linalg.norm(b))


def enet_kkt(D, q, rho, l1, l2, w):
    """max_j violation of the lasso / elastic-net optimality conditions, g = D^T D w + (l2/rho) w - q:
    g_j + kappa_j sign(w_j) = 0 where w_j != 0, |g_j| <= kappa_j where w_j = 0"""
    d = D.shape[1]
    l1 = np.broadcast_to(np.asarray(0.0 if l1 is None else l1, dtype=np.float64), (d,))
    l2 = np.broadcast_to(np.asarray(0.0 if l2 is None else l2, dtype=np.float64), (d,))
    kap = l1 / (2.0 * rho)
    g = D.T @ (D @ w) + (l2 / rho) * w - q
    r = np.where(w != 0, g + kap * np.sign(w), np.sign(g) * np.maximum(np.abs(g) - kap, 0.0))
    return float(np.max(np.abs(r)))


def ridge_exact_wide(D, q, rho, b):
    """(rho D^T D + diag(b)) w = rho q without a d x d matrix: the n x n identity on the coordinates with b_j > 0, a Schur
    complement on the (few) coordinates with b_j = 0.  D: scipy sparse n x d."""
    D = sp.csr_matrix(D)
    n, d = D.shape
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), (d,))
    P, F = np.flatnonzero(b > 0), np.flatnonzero(b == 0)
    DP = D[:, P]
    binv = 1.0 / b[P]
    K = sla.cho_factor(np.eye(n) / rho + (DP.multiply(binv[None, :]) @ DP.T).toarray())

    def solve_P(R):       # (rho DP^T DP + B_P)^-1 R for the columns of R
        t = binv[:, None] * R
        return t - binv[:, None] * (DP.T @ sla.cho_solve(K, DP @ t))

    rhs = rho * q
    w = np.zeros(d)
    if F.size == 0:
        w[P] = solve_P(rhs[P][:, None])[:, 0]
        return w
    DF = D[:, F].toarray()
    A_PF = rho * (DP.T @ DF)                      # |P| x |F|
    A_FF = rho * (DF.T @ DF)
    both = solve_P(np.concatenate([A_PF, rhs[P][:, None]], axis=1))     # one factorisation, |F| + 1 right-hand sides
    Z, y = both[:, :-1], both[:, -1]              # A_PP^-1 A_PF, A_PP^-1 rhs_P
    S = A_FF - A_PF.T @ Z
    wF = np.linalg.solve(S, rhs[F] - A_PF.T @ y)
    w[F] = wF
    w[P] = y - Z @ wF
    return w


def penalty_value(w, l1, l2):
    return 0.5 * float(np.sum(l1 * np.abs(w)) + np.sum(l2 * w * w))


def admm(D, weight_function, loss, l1, l2, reg0, args=None, iters=10):
    """The ADMM iteration of oracle/admm.py (mode "exact") on a sparse D = -y [X | 1] with per-coordinate penalties l1 / l2
    (d values each), never forming D^T D: the z-step is the oracle's, the ridge w-step is ridge_exact_wide, the elastic-net
    w-step the restated FISTA run to 1e-14.  reg0 sets the reference's starting values.  -> dict(w, z, lam, rho, objective)"""
    D = sp.csr_matrix(D)
    n, d = D.shape
    sa, sb = _w.get_weights(weight_function, n, args)
    lam = 0.1 * reg0 / n * np.ones(n)
    z = lam.copy()
    w = 0.001 * reg0 / d / n * np.ones(d)
    rho = _admm.initial_rho(weight_function)
    any_l1 = bool(np.any(l1 > 0))
    L = power_L(D) if any_l1 else None
    v = D @ w
    for _ in range(iters):
        m = v - lam / rho
        z, _ = _admm.z_step_exact(weight_function, loss, sa, sb, None, rho, m)
        q = D.T @ (z + lam / rho)
        if any_l1:
            w, _, ok = fista(D, q, rho, l1=l1, l2=l2, L=L, w0=w, tol=1e-14, max_iter=400000)
            assert ok, "the reference FISTA did not converge"
        else:
            w = ridge_exact_wide(D, q, rho, l2)
        v = D @ w
        lam = lam + rho * (z - v)
        primal = float(np.linalg.norm(z - v))
        rho = _admm.next_rho(rho, primal, d)
    obj = _obj.objective_from_v(loss, sa, v, w, None, None) + penalty_value(w, l1, l2)
    return dict(w=w, z=z, lam=lam, rho=rho, objective=obj)


# ---- the shapes of tests/test_gpu_wstep_op.py
def small_matrix(seed=0):
    """300 x 37 (ld = 40: the padding is live), about 20 % dense, row 5 empty, column 11 empty, column 36 all ones"""
    A = sp.random(300, 37, density=0.2, random_state=np.random.RandomState(seed), format="lil", dtype=np.float64)
    A[5, :] = 0.0
    A[:, 11] = 0.0
    A[:, 36] = 1.0
    A[5, 36] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def wide_matrix(n, d, per_row=6, seed=1, ones_column=False):
    """n x d with per_row entries in every row (most columns empty when n per_row << d); ones_column: the last column all ones"""
    rng = np.random.default_rng(seed)
    dd = d - 1 if ones_column else d
    cols = np.stack([np.sort(rng.choice(dd, size=per_row, replace=False)) for _ in range(n)])
    vals = rng.standard_normal((n, per_row))
    if ones_column:
        cols = np.concatenate([cols, np.full((n, 1), d - 1)], axis=1)
        vals = np.concatenate([vals, np.ones((n, 1))], axis=1)
    k = cols.shape[1]
    A = sp.csr_matrix((vals.reshape(-1), cols.reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, d))
    A.sort_indices()
    return A
