"""NumPy restatement of the working-set lasso (csrc/wstep_ws.hip, csrc/wset_plan.h) and an independent solver for its
fixtures.  A helper, not a conftest: nothing in the package imports it.

    min 1/2 w'(D^T D + diag(l2)/rho) w - q'w + sum_j kappa_j |w_j|,    kappa_j = l1_j / (2 rho) or reg / (2 rho)

The loop: S a list of at most CAP columns, every j with w_j != 0 in S, the free coordinates (kappa_j = 0 given per
coordinate) in S from the start.
  solve   the restricted problem on (Gs, q_S) exactly (here: a sign-pattern active-set method in float64)
  scan    g = D^T (D w) + (l2/rho) w - q; column j outside S is a candidate when |g_j| - kappa_j > tol max(1, max|q|);
          per chunk of CHUNK columns the largest violation, ties to the smaller index; then up to SELECT chunk winners,
          largest first, ties to the smaller index (select); none: done
  grow    append them (evicting the slots with w = 0 that are not free when S is full; still full: give up)

independent_lasso is another algorithm altogether - cyclic coordinate descent over the sparse columns with an
active-set schedule, then one linear solve on the support it found - and enet_kkt (wstep_op_ref) is the arbiter."""
import numpy as np
import scipy.sparse as sp

import wstep_op_ref as opref

CHUNK = opref.CHUNK   # wstep_op_plan.h: OP_CHUNK
CAP = 1024            # wset_plan.h: WS_CAP
SELECT = 64           # wset_plan.h: WS_SELECT
MAX_ROUNDS = CAP + 64  # wset_plan.h: WS_MAX_ROUNDS
FS_MAX = 96           # lasso_fs.hip: the active-set kernel's capacity
RHO = 0.37


# ---------------------------------------------------------------------------------------------------- the selection rule
def select(g, kappa, member, d=None, q=None, tol=1e-13, take=SELECT):
    """the scan's choice as the kernels make it: chunk by chunk, then winner by winner"""
    g, kappa = np.asarray(g, dtype=np.float64), np.asarray(kappa, dtype=np.float64)
    ld = g.size
    d = ld if d is None else d
    qmax = 0.0 if q is None else float(np.max(np.abs(q)))
    thr = tol * max(1.0, qmax)
    winners = []
    for c0 in range(0, ld, CHUNK):
        best, bj = None, None
        for j in range(c0, min(c0 + CHUNK, d)):
            if member[j]:
                continue
            v = abs(g[j]) - kappa[j]
            if best is None or v > best:      # ascending j: the smaller index among equals stays
                best, bj = v, j
        if best is not None and best > thr:
            winners.append((best, bj))
    out = []
    while winners and len(out) < take:
        k = 0
        for i in range(1, len(winners)):
            if winners[i][0] > winners[k][0] or (winners[i][0] == winners[k][0] and winners[i][1] < winners[k][1]):
                k = i
        out.append(winners.pop(k)[1])
    return out


def select_brute(g, kappa, member, d=None, q=None, tol=1e-13, take=SELECT):
    """the rule stated once more, with sorts: candidates -> the best of each chunk -> the first `take` by (-v, j)"""
    g, kappa = np.asarray(g, dtype=np.float64), np.asarray(kappa, dtype=np.float64)
    ld = g.size
    d = ld if d is None else d
    thr = tol * max(1.0, 0.0 if q is None else float(np.max(np.abs(q))))
    v = np.abs(g) - kappa
    cand = [j for j in range(d) if not member[j] and v[j] > thr]
    per_chunk = {}
    for j in sorted(cand, key=lambda j: (-v[j], j)):
        per_chunk.setdefault(j // CHUNK, j)
    return sorted(per_chunk.values(), key=lambda j: (-v[j], j))[:take]


# ---------------------------------------------------------------------------------------------------- the restricted solve
def dense_lasso_exact(G, q, kap, w0=None):
    """min 1/2 w'G w - q'w + sum kap_j |w_j| for a small positive definite G (any diagonal shift included), exactly: solve
    on the active set with its sign pattern, step to the first sign change, drop what hit zero; activate the largest
    violation.  kap_j = 0: a free coordinate, always active."""
    m = q.size
    w = np.zeros(m) if w0 is None else np.array(w0, dtype=np.float64)
    free = kap == 0.0
    act = (w != 0.0) | free
    theta = np.where(free, 0.0, np.sign(w))
    scale = max(1.0, float(np.max(np.abs(q))) if m else 1.0)
    for _ in range(20 * m + 100):
        for _ in range(4 * m + 20):
            A = np.flatnonzero(act)
            if A.size == 0:
                break
            x = np.linalg.solve(G[np.ix_(A, A)], q[A] - kap[A] * theta[A])
            wa = w[A]
            cross = (~free[A]) & (wa != 0.0) & (x * wa <= 0.0) & (x != wa)
            newcomer = (~free[A]) & (wa == 0.0) & (x * theta[A] <= 0.0)      # entered with a sign it cannot keep
            if not cross.any() and not newcomer.any():
                w[A] = x
                theta[A] = np.where(free[A], 0.0, np.sign(x))
                zero = (~free[A]) & (x == 0.0)
                act[A[zero]] = False
                break
            if newcomer.any():
                act[A[newcomer]] = False
                theta[A[newcomer]] = 0.0
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(cross, wa / (wa - x), np.inf)
            k = int(np.argmin(t))
            w[A] = wa + t[k] * (x - wa)
            hit = cross & (t <= t[k])
            w[A[hit]] = 0.0
            act[A[hit]] = False
            theta[A[hit]] = 0.0
        g = G @ w - q
        viol = np.where(act, -np.inf, np.abs(g) - kap)
        j = int(np.argmax(viol)) if m else 0
        if m == 0 or not viol[j] > 1e-14 * scale:
            return w
        act[j] = True
        theta[j] = -np.sign(g[j])
    raise AssertionError("dense_lasso_exact: no convergence")


# ---------------------------------------------------------------------------------------------------- the loop
def _vectors(d, rho, reg, l1, l2):
    pen = l1 is not None or l2 is not None
    l1v = np.broadcast_to(np.asarray(0.0 if l1 is None else l1, dtype=np.float64), (d,)) if pen else None
    l2v = np.broadcast_to(np.asarray(0.0 if l2 is None else l2, dtype=np.float64), (d,)) if pen else np.zeros(d)
    kap = l1v / (2.0 * rho) if pen else np.full(d, reg / (2.0 * rho))
    free = (l1v == 0.0) if pen else np.zeros(d, dtype=bool)
    return kap, np.asarray(l2v) / rho, free


def working_set_lasso(D, q, rho, reg=0.0, l1=None, l2=None, w0=None, tol=1e-13, cap=CAP, state=None):
    """-> (w, report).  state: a dict kept across calls on one D (S and Gs: the working set of a sequence of w-steps)"""
    D = sp.csc_matrix(D)
    d = D.shape[1]
    kap, sh, free = _vectors(d, rho, reg, l1, l2)
    w = np.zeros(d) if w0 is None else np.array(w0, dtype=np.float64)
    st = state if state is not None else {}
    if "S" not in st:
        st["S"], st["Gs"] = [], np.zeros((0, 0))
    rep = dict(rounds=0, pass_pairs=0, rows_last=0, evictions=0, left_route=0)

    def add(cols):
        S = st["S"]
        new = D[:, cols]
        old = D[:, S] if S else sp.csc_matrix((D.shape[0], 0))
        B = (old.T @ new).toarray()
        C = (new.T @ new).toarray()
        st["Gs"] = np.block([[st["Gs"], B], [B.T, C]])
        S.extend(int(c) for c in cols)
        rep["rows_last"] += len(cols)

    need = [j for j in range(d) if (free[j] or w[j] != 0.0) and j not in set(st["S"])]
    if len(st["S"]) + len(need) > cap:
        st["S"], st["Gs"] = [], np.zeros((0, 0))
        need = [j for j in range(d) if free[j]]
        sup = [j for j in range(d) if not free[j] and w[j] != 0.0]
        if len(need) + len(sup) <= cap:
            need += sup
        else:
            w[:] = 0.0
    if need:
        add(need)
    for rnd in range(MAX_ROUNDS):
        rep["rounds"] = rnd + 1
        S = np.array(st["S"], dtype=np.int64)
        if S.size:
            w[S] = dense_lasso_exact(st["Gs"] + np.diag(sh[S]), q[S], kap[S], w[S])
        if np.any(w != 0.0):
            g = D.T @ (D @ w) + sh * w - q
            rep["pass_pairs"] += 1
        else:
            g = -q
        member = np.zeros(d, dtype=bool)
        member[S] = True
        chosen = select(g, kap, member, d, q, tol)
        if not chosen:
            return w, rep
        if len(st["S"]) + len(chosen) > cap:
            keep = [a for a, j in enumerate(st["S"]) if w[j] != 0.0 or free[j]]
            rep["evictions"] += len(st["S"]) - len(keep)
            st["Gs"] = st["Gs"][np.ix_(keep, keep)]
            st["S"] = [st["S"][a] for a in keep]
        room = cap - len(st["S"])
        if room == 0:
            break
        add(chosen[:room])
    rep["left_route"] = 1
    return w, rep


# ---------------------------------------------------------------------------------------------------- the independent solver
def independent_lasso(D, q, rho, reg=0.0, l1=None, l2=None, sweeps=200):
    """cyclic coordinate descent on the sparse columns (full sweeps that find the active coordinates, sweeps over those
    until they stand), then one linear solve on the support with its signs.  -> w"""
    D = sp.csc_matrix(D)
    n, d = D.shape
    kap, sh, free = _vectors(d, rho, reg, l1, l2)
    ip, ix, va = D.indptr, D.indices, D.data
    a = np.asarray(D.multiply(D).sum(axis=0)).reshape(-1) + sh
    w, v = np.zeros(d), np.zeros(n)
    live = np.flatnonzero(a > 0.0)

    def sweep(cols):
        big = 0.0
        for j in cols:
            r, x = ix[ip[j]:ip[j + 1]], va[ip[j]:ip[j + 1]]
            h = x @ v[r] + sh[j] * w[j] - q[j]
            z = a[j] * w[j] - h
            new = np.sign(z) * max(abs(z) - kap[j], 0.0) / a[j]
            if new != w[j]:
                v[r] += x * (new - w[j])
                big = max(big, abs(new - w[j]))
                w[j] = new
        return big

    for _ in range(sweeps):
        if sweep(live) <= 1e-11:
            break
        act = np.flatnonzero((w != 0.0) | (free & (a > 0.0)))
        for _ in range(20000):
            if sweep(act) <= 1e-12:
                break
    A = np.flatnonzero((w != 0.0) | (free & (a > 0.0)))
    if A.size:
        DA = D[:, A]
        GA = (DA.T @ DA).toarray() + np.diag(sh[A])
        x = np.linalg.solve(GA, q[A] - kap[A] * np.sign(w[A]))
        if np.all((np.sign(x) == np.sign(w[A])) | free[A]):
            w[A] = x
    return w


def active_block_eigs(D, w, rho, l2=None):
    A = np.flatnonzero(w != 0.0)
    DA = sp.csc_matrix(D)[:, A]
    G = (DA.T @ DA).toarray()
    if l2 is not None:
        G = G + np.diag(np.broadcast_to(np.asarray(l2, dtype=np.float64), (D.shape[1],))[A] / rho)
    ev = np.linalg.eigvalsh(G)
    return float(ev[0]), float(ev[-1])


# ---------------------------------------------------------------------------------------------------- the fixtures
SHAPES = ((500, 2047), (500, 2048), (500, 2049), (500, 4097), (3000, 16385), (3000, 20000))
B_SEED = 7
KAPPA_FRAC = 0.05          # kappa = 0.05 max|q|: supports of 32 .. 77 (the issue's table)
OVERFLOW = (500, 4097, 0.03)   # support past FS_MAX


def fixture(n, d):
    """(D, q): wide_matrix(n, d, per_row=6, seed=d, ones_column=True), q = D^T b, b = default_rng(7).standard_normal(n) -
    the draw behind the supports 41 / 43 / 41 / 32 / 77 / 64 at kappa = 0.05 max|q|"""
    A = opref.wide_matrix(n, d, per_row=6, seed=d, ones_column=True)
    q = A.T @ np.random.default_rng(B_SEED).standard_normal(n)
    return A, q


def overflow_l2(d):
    return RHO * np.random.default_rng(d + 7).uniform(0.5, 2.0, d)
