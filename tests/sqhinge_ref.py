"""NumPy restatement of the squared hinge loss for the tests (a helper, not a conftest; the CPU oracle under oracle/
knows the reference's two losses only and stays as it is).

Convention of the library: D = -y * X, v = D w.
    loss    l(v)  = max(0, 1 + v)^2,       l'(v) = 2 max(0, 1 + v)
    prox    argmin_z sigma l(z) + rho/2 (z - m)^2 :  z = m                                  if m <= -1
                                                     z = (rho m - 2 sigma) / (rho + 2 sigma) otherwise
            (sigma = 0 returns m itself: rho m / rho may be an ulp off)
    block   root of Psi(t) = S l'(t) + rho (N t - M) (S = sum sigma, M = sum m, N elements):
                                                     t = M / N                               if M / N <= -1
                                                     t = (rho M - 2 S) / (rho N + 2 S)       otherwise
The z-step is the isotonic problem min sum_i sigma_i l(z_i) + rho/2 (z_i - m_i)^2 s.t. z non-decreasing along sorted m,
solved here by a stack PAV (pool adjacent violators; only a strict decrease violates).  For rank weights that are
constant on a few bands the same solution is clamp(prox, lo, hi) with the block values at the band edges as clamps
(`zstep_banded`): the identity the device's sort-free z-step relies on.

`admm` is the loop of oracle/admm.py in its exact mode for this loss, with the oracle's weights, w-steps, initial rho and
rho schedule unchanged.
"""
import numpy as np

from oracle import weights as _w
from oracle import wstep as _ws
from oracle.admm import initial_rho, next_rho

NAME = "squared_hinge"


def loss(v):
    t = np.maximum(1.0 + np.asarray(v), 0.0)
    return t * t


def dloss(v):
    return 2.0 * np.maximum(1.0 + np.asarray(v), 0.0)


def prox(sigma, rho, m):
    m = np.asarray(m)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=m.dtype), m.shape)
    return np.where((m <= -1.0) | (sigma == 0.0), m, (rho * m - 2.0 * sigma) / (rho + 2.0 * sigma))


def block_value(S, M, N, rho):
    """root of Psi for a pooled block (scalars)"""
    if M / N <= -1.0 or S == 0.0:
        return M / N
    return (rho * M - 2.0 * S) / (rho * N + 2.0 * S)


def psi(S, M, N, rho, t):
    return S * 2.0 * max(1.0 + t, 0.0) + rho * (N * t - M)


def pav(sigma, rho, m_sorted, return_blocks=False):
    """Stack PAV on sorted m.  Returns z (and the blocks as (start, end_exclusive, S, M, value))."""
    m = np.asarray(m_sorted)
    dt = m.dtype.type
    sg = np.broadcast_to(np.asarray(sigma, dtype=m.dtype), m.shape)
    u0 = prox(sg, rho, m)
    rho = dt(rho)
    st_s, st_S, st_M, st_x = [], [], [], []       # block start, sum sigma, sum m, value
    for i in range(m.shape[0]):
        s, S, M, x = i, sg[i], m[i], u0[i]
        while st_s and st_x[-1] > x:              # only a strict decrease violates
            s = st_s.pop()
            S = st_S.pop() + S
            M = st_M.pop() + M
            st_x.pop()
            x = block_value(S, M, dt(i + 1 - s), rho)
        st_s.append(s)
        st_S.append(S)
        st_M.append(M)
        st_x.append(x)
    z = np.empty_like(m)
    ends = st_s[1:] + [m.shape[0]]
    for s, e, x in zip(st_s, ends, st_x):
        z[s:e] = x
    if return_blocks:
        return z, [(s, e, S, M, x) for s, e, S, M, x in zip(st_s, ends, st_S, st_M, st_x)]
    return z


def bands_of(sigma):
    """[(start, end_exclusive, value)] of a piecewise-constant weight vector"""
    sigma = np.asarray(sigma)
    cuts = [0] + (np.flatnonzero(sigma[1:] != sigma[:-1]) + 1).tolist() + [sigma.shape[0]]
    return [(a, b, float(sigma[a])) for a, b in zip(cuts[:-1], cuts[1:])]


def zstep_banded(sigma, rho, m_sorted):
    """The z-step for banded sigma WITHOUT pooling adjacent violators: inside a band the prox is monotone in m, so the
    isotonic solution pools only across band edges, one block per edge between two bands of several ranks (the top of the
    band below with u > x, the single-rank bands in between, the bottom of the band above with u < x; x the root of the
    pooled Psi), and z = clamp(prox, lo, hi) with those block values.  Returns (z, block values) or None where the
    structure cannot be certified (a block that swallows an inner band, stays on one side of a single-rank band, or two
    blocks that meet inside a band) - the device redoes such a step with the sort + PAV."""
    m = np.asarray(m_sorted, dtype=np.float64)
    n = m.shape[0]
    bands = bands_of(sigma)
    u = prox(np.asarray(sigma, dtype=np.float64), rho, m)
    nb = len(bands)
    multi = [j for j, (a, b, _) in enumerate(bands) if b - a > 1 or j == 0 or j == nb - 1]
    lo = np.full(nb, -np.inf)
    hi = np.full(nb, np.inf)
    xs = []
    for L, R in zip(multi[:-1], multi[1:]):
        aL, bL, sL = bands[L]
        aR, bR, sR = bands[R]
        chain = [u[bL - 1]] + [u[bands[j][0]] for j in range(L + 1, R)] + [u[aR]]
        if all(c1 <= c2 for c1, c2 in zip(chain[:-1], chain[1:])):
            continue                                            # nothing to pool at this edge
        St = sum(bands[j][2] for j in range(L + 1, R))
        Mt = sum(m[bands[j][0]] for j in range(L + 1, R))
        nt = R - L - 1
        uL, uR = u[aL:bL], u[aR:bR]

        def sets(x):
            iT = aL + int(np.searchsorted(uL, x, side="right"))     # first position of L with u > x
            iB = aR + int(np.searchsorted(uR, x, side="left"))      # first position of R with u >= x
            cT, cB = bL - iT, iB - aR
            return iT, iB, sL * cT + St + sR * cB, m[iT:bL].sum() + Mt + m[aR:iB].sum(), cT + nt + cB

        a, b = min(chain), max(chain)
        x = None
        for _ in range(200):                                    # Psi is increasing: bisect until the set repeats
            t = 0.5 * (a + b)
            iT, iB, S, M, N = sets(t)
            xt = block_value(S, M, float(N), rho)
            if sets(xt)[:2] == (iT, iB):
                x = xt
                break
            if psi(S, M, float(N), rho, t) > 0.0:
                b = t
            else:
                a = t
        if x is None:
            return None
        iT, iB, S, M, N = sets(x)
        cT, cB = bL - iT, iB - aR
        if (cT == bL - aL and L != 0) or (cB == bR - aR and R != nb - 1):
            return None                                         # a whole inner band swallowed
        if nt == 0:
            ok = cT > 0 and cB > 0
        else:
            u1, u2 = u[bands[L + 1][0]], u[bands[R - 1][0]]
            if cT > 0 and cB > 0:
                ok = True
                if nt == 2:
                    m1, s1 = m[bands[L + 1][0]], bands[L + 1][2]
                    m2, s2 = m[bands[R - 1][0]], bands[R - 1][2]
                    xl = block_value(sL * cT + s1, m[iT:bL].sum() + m1, cT + 1.0, rho)
                    xr = block_value(s2 + sR * cB, m2 + m[aR:iB].sum(), 1.0 + cB, rho)
                    ok = xl >= x and xr <= x
            elif cT > 0:
                ok = u2 <= x
            else:
                ok = u1 >= x
        if not ok:
            return None
        hi[L] = x
        lo[R] = x
        for j in range(L + 1, R):
            lo[j] = hi[j] = x
        xs.append(x)
    if np.any(lo > hi):
        return None
    z = np.empty(n)
    for j, (a, b, _) in enumerate(bands):
        z[a:b] = np.clip(u[a:b], lo[j], hi[j])
    return z, xs


def z_step(weight_function, sigma, rho, m):
    if weight_function == "erm":
        return prox(sigma, rho, m)
    order = np.argsort(m, kind="stable")
    z = np.empty_like(m)
    z[order] = pav(sigma, rho, m[order])
    return z


def objective_from_v(sigma, v, w, l2_reg=None, l1_reg=None):
    risk = float(np.dot(sigma, np.sort(loss(np.asarray(v, dtype=np.float64)))))
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if l2_reg:
        risk += 0.5 * l2_reg * float(np.sum(w ** 2))
    if l1_reg:
        risk += 0.5 * l1_reg * float(np.sum(np.abs(w)))
    return risk


class Trace(dict):
    __getattr__ = dict.__getitem__


def admm(X, y, weight_function="erm", l2_reg=None, l1_reg=None, args=None, w0=None, max_iter=200, tol=1e-4,
         smooth=False, t=1.0, w_tol=1e-14, ridge_in_n_space=False):
    """oracle/admm.py:admm_solve(mode='exact') for the squared hinge: same state initialisation, w-steps, residuals,
    stop rule, rho schedule and smoothing schedule; only the z-step and the objective are this file's.

    ridge_in_n_space (l2 only, meant for n << d): the ridge system (rho G + reg I) w = rho q has q = D^T b with
    b = z + lambda / rho, so its solution is w = D^T a with (rho D D^T + reg I) a = rho b - multiply that by D^T.  The
    identity is exact and loses nothing (the n x n matrix has the condition of the d x d one on the row space of D), and
    at d = 16 000 it replaces a 2 GB Gram matrix and a d^3 solve per iteration by n^3 work; the host tests hold it to
    oracle.wstep.ridge_gram_exact."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    sigma, _ = _w.get_weights(weight_function, n, args)
    D = -np.asarray(y, dtype=np.float64).reshape(-1, 1) * X
    reg = l1_reg or l2_reg
    lam = 0.1 * reg / n * np.ones(n)
    z = 0.1 * reg / n * np.ones(n)
    w = (np.asarray(w0, dtype=np.float64).reshape(-1).copy() if w0 is not None else 0.001 * reg / d / n * np.ones(d))
    rho = initial_rho(weight_function)
    w_flag = 1 if l1_reg is not None else 2
    if ridge_in_n_space:
        assert w_flag == 2
        K = D @ D.T
    else:
        G = D.T @ D
        L = 1.0001 * _ws.lambda_max(G)

    def F(wv, v=None):
        return objective_from_v(sigma, D @ wv if v is None else v, wv, l2_reg, l1_reg)

    tr = Trace(primal=[], dual=[], rho=[], objective=[F(w)])
    v = D @ w
    converged = False
    it = 0
    for it in range(max_iter):
        m = v - lam / rho
        z = z_step(weight_function, sigma, rho, m)
        pre_w = w.copy()
        q = None if ridge_in_n_space else D.T @ (z + lam / rho)
        if ridge_in_n_space:
            w = D.T @ np.linalg.solve(rho * K + reg * np.eye(n), rho * (z + lam / rho))
        elif w_flag == 1 and not smooth:
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
        if primal < tol and dual < tol:
            converged = True
            break
        rho = next_rho(rho, primal, d)
        tr.objective.append(F(w, v))
        if smooth and it >= 17:
            t = max(t * 0.9, 1e-9) % np.power(rho, -0.1) * np.power(float(it), -0.1)
    if smooth and w_flag == 1:
        w = np.sign(w) * np.where((np.abs(w) - t) > 0, np.abs(w) - t, 0)
    tr.update(w=w, z=z, lam=lam, rho_final=rho, iters=it + 1, converged=converged, final_objective=F(w), t=t, n=n, d=d,
              sigma=sigma, D=D)
    return tr
