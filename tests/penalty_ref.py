"""NumPy reference for the w-step with per-coordinate penalties (include/rbl.h: rbl_set_penalty)

    min_w  1/2 w'(G + diag(l2)/rho) w - q'w + sum_j kappa_j |w_j|,      kappa_j = l1_j / (2 rho)

and its optimality conditions.  Test infrastructure only: nothing in the package imports it."""
import numpy as np


def _parts(G, q, rho, l1, l2):
    d = np.asarray(q).size
    l1 = np.zeros(d) if l1 is None else np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,))
    l2 = np.zeros(d) if l2 is None else np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,))
    return np.asarray(G, dtype=np.float64) + np.diag(l2 / rho), l1 / (2.0 * rho)


def enet_kkt_residual(G, q, rho, l1, l2, w):
    """max_j of the violation of: g_j + kappa_j sign(w_j) = 0 where w_j != 0, |g_j| <= kappa_j where w_j = 0,
    with g = G w + (l2/rho) w - q."""
    Gs, kap = _parts(G, q, rho, l1, l2)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    g = Gs @ w - np.asarray(q, dtype=np.float64).reshape(-1)
    r = np.where(w != 0, g + kap * np.sign(w), np.sign(g) * np.maximum(np.abs(g) - kap, 0.0))
    return float(np.max(np.abs(r)))


def enet_objective(G, q, rho, l1, l2, w):
    Gs, kap = _parts(G, q, rho, l1, l2)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    return float(0.5 * w @ (Gs @ w) - np.asarray(q).reshape(-1) @ w + np.sum(kap * np.abs(w)))


def enet_gram_exact(G, q, rho, l1, l2, w0=None, tol=1e-14, max_iter=200000):
    """FISTA with gradient restart (fixed step 1 / lambda_max, per-coordinate soft threshold) run until the iterate
    moves by less than tol, then an active-set polish: with the support and the signs FISTA found, the minimiser solves
    a linear system on the support (free coordinates, kappa_j = 0, always belong to it); the solve is kept when it
    preserves the signs and lowers the KKT residual."""
    Gs, kap = _parts(G, q, rho, l1, l2)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    d = q.size
    w = np.zeros(d) if w0 is None else np.array(w0, dtype=np.float64).reshape(-1)
    L = 1.0001 * float(np.linalg.eigvalsh(Gs)[-1])
    if not L > 0:
        L = 1.0
    yk, t = w.copy(), 1.0
    for _ in range(max_iter):
        b = yk - (Gs @ yk - q) / L
        wn = np.sign(b) * np.maximum(np.abs(b) - kap / L, 0.0)
        dw = wn - w
        if np.dot(yk - wn, dw) > 0:
            t, yk = 1.0, wn.copy()
        else:
            tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
            yk = wn + ((t - 1.0) / tn) * dw
            t = tn
        w = wn
        if np.max(np.abs(dw)) <= tol * max(1.0, np.max(np.abs(w))):
            break
    for _ in range(3):
        A = (w != 0) | (kap == 0)
        if not A.any():
            break
        theta = np.sign(w[A])
        x = np.linalg.lstsq(Gs[np.ix_(A, A)], q[A] - kap[A] * theta, rcond=None)[0]
        cand = np.zeros(d)
        cand[A] = x
        same_sign = np.all((np.sign(x) == theta) | (kap[A] == 0))
        if same_sign and enet_kkt_residual(G, q, rho, l1, l2, cand) < enet_kkt_residual(G, q, rho, l1, l2, w):
            w = cand
        else:
            break
    return w
