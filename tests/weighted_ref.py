"""Row-weighted erm on the CPU (a helper, not a conftest): the erm loop of oracle/admm.py restated with
sigma_i = c_i * (1 / n),
    min_w (1/n) sum_i c_i loss(D_i w) + R(w),
built from the oracle's own parts - oracle.prox.prox_exact (sqhinge_ref.prox for the squared hinge), oracle.wstep.*,
initial_rho and next_rho.  Only the z-step and the logged objective see the weights; everything else is admm_solve's
"exact" mode line by line, so c == 1 returns its iterates bit for bit (tests/test_row_weights_host.py).

``c`` may be a dict {iteration: weights}: the weights are switched at the START of that iteration (key 0 = the
initial ones; a value None = unweighted from there on), which is what Solver.set_row_weights between two steps does."""
import math

import numpy as np

from oracle import prox as _oprox
from oracle import wstep as _ws
from oracle.admm import Trace, initial_rho, next_rho
import sqhinge_ref


def sample_losses(loss, v):
    v = np.asarray(v, dtype=np.float64)
    if loss == "binary_cross_entropy":
        return _oprox.softplus(v)
    if loss == "hinge":
        return np.maximum(1.0 + v, 0.0)
    if loss == "squared_hinge":
        return sqhinge_ref.loss(v)
    raise ValueError(loss)


def prox(loss, sigma, rho, m):
    if loss == "squared_hinge":
        return sqhinge_ref.prox(sigma, rho, m)
    return _oprox.prox_exact(loss, sigma, rho, m)


def reg_term(w, l2_reg=None, l1_reg=None):
    r = 0.0
    if l2_reg:
        r += 0.5 * l2_reg * float(np.sum(w ** 2))
    if l1_reg:
        r += 0.5 * l1_reg * float(np.sum(np.abs(w)))
    return r


def objective(loss, c, v, w, l2_reg=None, l1_reg=None):
    """F(w) = (1/n) sum_i c_i loss(v_i) + R(w), the sum in exact arithmetic (math.fsum)"""
    n = v.shape[0]
    c = np.ones(n) if c is None else np.asarray(c, dtype=np.float64)
    return math.fsum((c * sample_losses(loss, v)).tolist()) / n + reg_term(np.asarray(w, dtype=np.float64), l2_reg, l1_reg)


def admm(X, y, c, loss="binary_cross_entropy", l2_reg=None, l1_reg=None, max_iter=200, tol=1e-4, smooth=False, t=1.0,
         w_tol=1e-14, D=None):
    """oracle.admm.admm_solve(weight_function="erm", mode="exact") with row weights c (n values, None, or a dict
    {iteration: weights}).  D: the stored matrix (-y * X rounded to the storage type) to run on instead of -y * X."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    D = -np.asarray(y).reshape(-1, 1) * X if D is None else np.asarray(D, dtype=np.float64)
    G = D.T @ D
    sched = c if isinstance(c, dict) else {0: c}
    sigma0 = 1.0 / n

    def sigma_of(cw):
        return np.full(n, sigma0) if cw is None else np.asarray(cw, dtype=np.float64) * sigma0   # the ONE product

    cw = sched.get(0)
    sigma = sigma_of(cw)
    reg = l1_reg or l2_reg
    lam = 0.1 * reg / n * np.ones(n)
    z = 0.1 * reg / n * np.ones(n)
    w = 0.001 * reg / d / n * np.ones(d)
    rho = initial_rho("erm")
    w_flag = 1 if l1_reg is not None else 2
    L = 1.0001 * _ws.lambda_max(G)
    tr = Trace(primal=[], dual=[], rho=[], objective=[objective(loss, cw, D @ w, w, l2_reg, l1_reg)], states=[])
    v = D @ w
    converged = False
    it = 0
    for it in range(max_iter):
        if it in sched and it > 0:
            cw = sched[it]
            sigma = sigma_of(cw)
        m = v - lam / rho
        z = prox(loss, sigma, rho, m)
        pre_w = w.copy()
        q = D.T @ (z + lam / rho)
        if w_flag == 1 and not smooth:
            w, _ = _ws.lasso_gram_exact(G, q, reg / (2.0 * rho), w, L, tol=w_tol)
        elif w_flag == 1:
            w, _ = _ws.smooth_l1_gram_exact(G, q, rho, reg, t, w, L, tol=w_tol)
        else:
            w = _ws.ridge_gram_exact(G, q, rho, reg)
        v = D @ w
        lam = lam + rho * (z - v)
        primal = float(np.linalg.norm(z - v))
        dual = float(np.linalg.norm(w - pre_w))
        tr.primal.append(primal)
        tr.dual.append(dual)
        tr.rho.append(rho)
        tr.states.append((w.copy(), z.copy(), lam.copy()))
        if primal < tol and dual < tol:
            converged = True
            break
        rho = next_rho(rho, primal, d)
        tr.objective.append(objective(loss, cw, v, w, l2_reg, l1_reg))
        if smooth and it >= 17:
            t = max(t * 0.9, 1e-9) % np.power(rho, -0.1) * np.power(float(it), -0.1)
    if smooth and w_flag == 1:
        w = np.sign(w) * np.where((np.abs(w) - t) > 0, np.abs(w) - t, 0)
    tr.update(w=w, z=z, lam=lam, rho_final=rho, iters=it + 1, converged=converged, t=t, n=n, d=d, D=D)
    return tr
