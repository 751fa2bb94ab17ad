"""Reference, inputs and instance table for the row-streaming passes (csrc/sweep_erm.hip, csrc/sweep_multi.hip) run
through the rbl_k_sweep_* entry points with a chosen grid (a helper, not a conftest).

Reference: lines 5-9 of the header of sweep_erm.hip, per row, in NumPy float64 -
    v = D w,  res = z_old - v,  lam' = lam + rho res,  m = v - lam' / rho_next,  z' = prox(sigma0, rho_next, m),
    c = z' + lam' / rho_next,  q = D^T c,  primal2 = sum res^2,  zz = sum z'^2
with D rounded to the storage type first.  The V-only pass is the first three and primal2, the Q-only pass q = D^T c.

Launch geometry: a wave (a workgroup of the wide kernel) takes the super-batches gw, gw + GW, ... of S*R rows.  TABLE
restates, as data, which instance (kind, P | PT, R, S) the launch tables pick per range of 16-byte packets per row; the
GPU tests assert that the instance a call reports is the table's, so a change of the dispatch has to change the table.

Two families of inputs:
  dyadic       D in k/8 (|k| <= 16), vectors in multiples of 1/4, rho / rho_next / sigma0 powers of two: every
               intermediate, the sums of squares included, is exact in 53 bits in ANY order of summation, so the device
               must return the reference's bits.  The reference is computed in integers as well and must agree.
  real-valued  standard normal D, w, z, lam; bounds propagated through the formulas from the project's two constants
               (1e-13 x (absolute sum + 1) for an fp64 dot product or column sum: test_gemv_gemvt; 1e-12 x max(1, |ref|)
               for the prox root: test_prox_vs_oracle) plus a few ulps per rounding.  The whole bound, with
               u(x) = 4 x 2^-52 |x| for one rounded operation on operands of size x (class Real):
                   e_v   = 1e-13 (|D| |w| + 1)
                   e_res = e_v + u(|z_old| + |v|)
                   e_lam = rho e_v + u(|lam| + rho (|z_old| + |v|))
                   e_lr  = e_lam / rho_next + u(lam' / rho_next)                    (the division)
                   e_m   = e_v + e_lr + u(|v| + |lam' / rho_next|)                  (the subtraction)
                   e_z   = e_m + 1e-12 max(1, max |z'|)                             (the prox is 1-Lipschitz in m)
                   e_c   = e_z + e_lr + u(|z'| + |lam' / rho_next|)                 (the addition)
                   e_q   = |D|^T e_c + 1e-13 (|D|^T |c| + 1)
                   e_primal2 = sum (2 |res| e_res + e_res^2) + 1e-13 (sum res^2 + 1),   e_zz likewise with z', e_z
               No other constant enters.  The u() terms also cover the rounding of the float64 reference itself.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import prox as _oprox
import sqhinge_ref

LOSSES = ("binary_cross_entropy", "hinge", "squared_hinge")
STORAGES = ("f32", "f64", "fp16")
PACKET = {"f32": 4, "f64": 2, "fp16": 8}          # elements per 16-byte packet
PAD = {"f32": 4, "f64": 4, "fp16": 8}             # the row stride is a multiple of this many elements
NP_DTYPE = {"f32": np.float32, "f64": np.float64, "fp16": np.float16}
WIDE_THREADS = 512

# ------------------------------------------------------------------------------------------------ the instance table
Inst = namedtuple("Inst", "pk_lo pk_hi kind p r s")   # packets per row in [pk_lo, pk_hi] -> (kind, P | PT, R, S)

_FUSED_WAVE = [Inst(33, 64, "wave", 1, 16, 2), Inst(65, 128, "wave", 2, 8, 8), Inst(129, 256, "wave", 4, 4, 4),
               Inst(257, 512, "wave", 8, 4, 4)]
_FUSED_WIDE = [Inst(513, 1024, "wide", 2, 8, 2), Inst(1025, 1536, "wide", 3, 6, 4), Inst(1537, 2048, "wide", 4, 4, 4),
               Inst(2049, 2560, "wide", 5, 3, 8), Inst(2561, 3072, "wide", 6, 2, 8), Inst(3073, 4096, "wide", 8, 1, 16)]
_FUSED_F16 = _FUSED_WAVE[:3] + [Inst(257, 512, "wide", 1, 16, 1), Inst(513, 1024, "wide", 2, 8, 2),
                                Inst(1025, 1536, "wide", 3, 4, 4), Inst(1537, 2048, "wide", 4, 2, 8)]
_HALF = [Inst(33, 64, "wave", 1, 8, 2), Inst(65, 128, "wave", 2, 4, 4), Inst(129, 256, "wave", 4, 2, 8),
         Inst(257, 512, "wave", 8, 2, 8)]
TABLE = {
    "fused": {"f32": _FUSED_WAVE + _FUSED_WIDE, "f64": _FUSED_WAVE + _FUSED_WIDE, "fp16": _FUSED_F16},
    "v": {"f32": _HALF, "f64": _HALF, "fp16": _HALF},
    "q": {"f32": _HALF, "f64": _HALF, "fp16": _HALF},
    "multi_v": {"f32": _HALF, "f64": _HALF, "fp16": _HALF[:3]},
    "multi_q": {"f32": _HALF, "f64": _HALF, "fp16": _HALF[:3]},
}
PASSES = tuple(TABLE)


def ld_of(d, storage):
    return -(-int(d) // PAD[storage]) * PAD[storage]


def packets(d, storage):
    return ld_of(d, storage) // PACKET[storage]


def lookup(pass_, storage, d):
    """the table's instance for width d, or None outside the pass' widths"""
    pk = packets(d, storage)
    for inst in TABLE[pass_][storage]:
        if inst.pk_lo <= pk <= inst.pk_hi:
            return inst
    return None


def blocks(pass_, inst, num_cu):
    """blocks launched: one per CU, two for the fused pass at one packet per lane"""
    return 2 * num_cu if (pass_ == "fused" and inst.kind == "wave" and inst.p == 1) else num_cu


def workers(pass_, inst, num_cu):
    """GW: waves (4 per block), or workgroups of the wide kernel, that share the super-batches"""
    b = blocks(pass_, inst, num_cu)
    return 4 * b if inst.kind == "wave" else b


def reported(pass_, inst, num_cu):
    """what a rbl_k_sweep_* call reports for this instance"""
    return (inst.kind, inst.p, inst.r, inst.s, blocks(pass_, inst, num_cu))


def widths(storage, inst):
    """the narrowest and the widest d that select the instance, and one below the widest (padded columns; the
    narrowest is padded as well)"""
    ld_min = -(-inst.pk_lo * PACKET[storage] // PAD[storage]) * PAD[storage]
    d_max = inst.pk_hi * PACKET[storage]
    return (ld_min - PAD[storage] + 1, d_max - 1, d_max)


def row_counts(pass_, inst, num_cu):
    """n per instance and grid: a single row; a tail inside the second sub-batch; around one super-batch; every worker
    exactly one super-batch; one worker loops for a single live row; third round with a ragged last super-batch whose
    last sub-batch is ragged too"""
    sr, gw = inst.s * inst.r, workers(pass_, inst, num_cu)
    return sorted({1, inst.r + 1, sr - 1, sr, sr + 1, gw * sr, gw * sr + 1, 2 * gw * sr + sr + inst.r + 1})


def looping_rows(pass_, inst, num_cu):
    """the two row counts at which a worker runs its loop again"""
    sr, gw = inst.s * inst.r, workers(pass_, inst, num_cu)
    return (gw * sr + 1, 2 * gw * sr + sr + inst.r + 1)


def max_super_batches(pass_, inst, num_cu, n):
    """super-batches of the busiest worker (worker 0)"""
    sr, gw = inst.s * inst.r, workers(pass_, inst, num_cu)
    return -(-(-(-n // sr)) // gw)


def n_max(pass_, inst):
    return max(row_counts(pass_, inst, 2))


def storage_round(X, storage):
    return np.asarray(X, dtype=np.float64).astype(NP_DTYPE[storage]).astype(np.float64)


def prox(loss, sigma0, rho, m):
    if loss == "squared_hinge":
        return sqhinge_ref.prox(sigma0, rho, m)
    return _oprox.prox_exact(loss, sigma0, rho, m)


# ------------------------------------------------------------------------------------------------ dyadic inputs
UNIT_LOG = 24                       # integer arithmetic in units of 2^-24
UNIT = 1 << UNIT_LOG
DYADIC_PARAMS = [(2.0, 4.0, 0.5), (0.5, 1.0, 0.25), (1.0, 2.0, 2.0)]   # (rho, rho_next, sigma0): powers of two
MULTI_RHO = (0.5, 1.0, 2.0, 4.0)
KINK_STEP = 2.0 ** -10


def _log2_exact(x):
    mant, e = math.frexp(x)
    assert mant == 0.5, f"{x} is no power of two"
    return e - 1


def _scale(num, x):
    """num * x for a power of two x, in integers; the division must be exact"""
    e = _log2_exact(x)
    if e >= 0:
        return num * (1 << e)
    assert not np.any(num % (1 << -e)), "a dyadic quantity left the integer grid"
    return num // (1 << -e)


def _to_units(x):
    num = np.asarray(x, dtype=np.float64) * UNIT
    assert np.all(num == np.round(num)) and np.all(np.abs(num) < 2.0 ** 62)
    return num.astype(np.int64)


def _from_units(num):
    return np.asarray(num, dtype=np.int64).astype(np.float64) / UNIT


def _trailing(nums):
    """the largest t with 2^t dividing every entry (63 for all zeros)"""
    g = 0
    for x in np.asarray(nums, dtype=object).reshape(-1).tolist():
        g = math.gcd(g, int(x))
    return 63 if g == 0 else (g & -g).bit_length() - 1


def any_order_exact(terms_abs_sum, grid_nums):
    """True when every partial sum, in any order, of terms whose absolute values sum to at most terms_abs_sum (integers
    on the grid of grid_nums) fits 53 bits"""
    t = _trailing(grid_nums)
    return (int(terms_abs_sum) >> t) < (1 << 53)


def _sq_prefix(num, counts):
    """exact prefix sums of num^2 (Python integers, units of 2^-48) -> {n: float, exactly}"""
    sq = [int(x) * int(x) for x in num.tolist()]
    t = _trailing(sq)                                        # the grid of the terms, hence of every partial sum
    out, acc, i = {}, 0, 0
    for n in sorted(counts):
        while i < n:
            acc += sq[i]
            i += 1
        assert (acc >> t) < (1 << 53), "a sum of squares does not fit 53 bits: shrink the magnitudes"
        out[n] = float(acc) / float(UNIT) / float(UNIT)
        assert int(out[n] * UNIT * UNIT) == acc
    return out


class Dyadic:
    """Inputs and exact reference of one (storage, width) for the fused pass with the hinge loss, the V-only and the
    Q-only pass; every row-wise quantity for n_rows rows, the sums for each n in counts."""

    def __init__(self, storage, d, n_rows, counts, seed):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.n, self.counts = storage, d, n_rows, tuple(sorted(counts))
        self.rho, self.rho_next, self.sigma0 = DYADIC_PARAMS[seed % len(DYADIC_PARAMS)]
        D8 = rng.integers(-16, 17, size=(n_rows, d))
        w4 = rng.integers(-4, 5, size=d)
        z4 = rng.integers(-8, 9, size=n_rows)
        l4 = rng.integers(-8, 9, size=n_rows)
        c4 = rng.integers(1, 9, size=n_rows) * rng.choice([-1, 1], size=n_rows)   # the Q-only coefficient: never 0
        w4[0] = 1                                                                 # a unit step of D[i, 0] moves v[i]
        z = z4 * (UNIT // 4)
        # hinge kinks at m = -1 and m - sigma0 / rho_next = -1: every seventh row gets the lambda that puts m on, just
        # below or just above one of them (lam = rho_next (v - m) - rho (z - v), all on the grid)
        s = _to_units(self.sigma0 / self.rho_next)
        g = _to_units(KINK_STEP)
        targets = [-UNIT, -UNIT - g, -UNIT + g, -UNIT + s, -UNIT + s - g, -UNIT + s + g]
        self.kink_rows = np.arange(3, n_rows, 7)
        while True:
            v32 = D8 @ w4                                                         # units of 1/32
            assert np.all(np.abs(D8) @ np.abs(w4) < 2 ** 53)
            v = v32 * (UNIT // 32)
            lam = l4 * (UNIT // 4)
            for k, i in enumerate(self.kink_rows):
                lam[i] = _scale(v[i] - targets[k % 6], self.rho_next) - _scale(z[i] - v[i], self.rho)
            # ---- the reference in integers
            res = z - v
            lam1 = lam + _scale(res, self.rho)
            lr = _scale(lam1, 1.0 / self.rho_next)
            m = v - lr
            a = m - s
            zn = np.where(a >= -UNIT, a, np.where(m <= -UNIT, m, -UNIT))
            c = zn + lr
            zero = c == 0
            if not zero.any():
                break
            # a row whose coefficient is 0 could be dropped unnoticed: move its v by 1/32 and start again
            D8[zero, 0] += np.where(D8[zero, 0] < 16, 1, -1)
        self.D8 = D8
        self.D, self.w, self.z_old, self.c_in = D8 / 8.0, w4 / 4.0, z4 / 4.0, c4 / 4.0
        assert np.array_equal(storage_round(self.D, storage), self.D)            # exact in every storage type
        self.lam = _from_units(lam)
        self.kink_m = m[self.kink_rows]
        assert np.array_equal(self.kink_m, np.array([targets[k % 6] for k in range(len(self.kink_rows))], dtype=np.int64))
        self.i_v, self.i_lam1, self.i_zn, self.i_c, self.i_res = v, lam1, zn, c, res
        self.ref = self._sums(v, lam1, zn, c, res, _to_units(self.c_in))
        # ---- the same in float64, as the header of sweep_erm.hip states it
        fv = self.D @ self.w
        fres = self.z_old - fv
        flam = self.lam + self.rho * fres
        flr = flam / self.rho_next
        fm = fv - flr
        fz = _oprox.prox_hinge_exact(self.sigma0, self.rho_next, fm)
        fc = fz + flr
        self.f64 = dict(v=fv, lam=flam, z=fz, c=fc,
                        q={n: self.D[:n].T @ fc[:n] for n in self.counts},
                        q_only={n: self.D[:n].T @ self.c_in[:n] for n in self.counts},
                        primal2={n: float(np.sum(fres[:n] ** 2)) for n in self.counts},
                        zz={n: float(np.sum(fz[:n] ** 2)) for n in self.counts})

    def _sums(self, v, lam1, zn, c, res, c_only):
        ref = dict(v=_from_units(v), lam=_from_units(lam1), z=_from_units(zn), c=_from_units(c))
        for x, name in ((v, "v"), (lam1, "lam"), (zn, "z"), (c, "c")):
            assert np.array_equal(_to_units(ref[name]), x)
        A = np.abs(self.D8)
        for name, coef in (("q", c), ("q_only", c_only)):
            t = _trailing(coef)
            cc = coef >> t                                   # D8 * cc: units of 2^-(27 - t)
            assert any_order_exact(int(np.max(A.T @ np.abs(cc))), [1]), "q does not fit 53 bits: shrink the magnitudes"
            ref[name] = {n: (self.D8[:n].T @ cc[:n]).astype(np.float64) * (2.0 ** (t - UNIT_LOG - 3)) for n in self.counts}
        ref["primal2"] = _sq_prefix(res, self.counts)
        ref["zz"] = _sq_prefix(zn, self.counts)
        return ref

    def exactness_report(self):
        """the integer reference against the float64 evaluation: a list of what differs (empty when exact)"""
        bad = []
        for name in ("v", "lam", "z", "c"):
            if not np.array_equal(self.ref[name], self.f64[name]):
                bad.append(name)
        for name in ("q", "q_only"):
            bad += [f"{name}[{n}]" for n in self.counts if not np.array_equal(self.ref[name][n], self.f64[name][n])]
        for name in ("primal2", "zz"):
            bad += [f"{name}[{n}]" for n in self.counts if self.ref[name][n] != self.f64[name][n]]
        return bad


class DyadicMulti:
    """k columns on one dyadic D: the V pass with the lambda update (a rho per column) and the Q pass"""

    def __init__(self, storage, d, n_rows, counts, seed, k=4):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.n, self.counts, self.k = storage, d, n_rows, tuple(sorted(counts)), k
        D8 = rng.integers(-16, 17, size=(n_rows, d))
        self.D8, self.D = D8, D8 / 8.0
        W4 = rng.integers(-4, 5, size=(k, d))
        Z4 = rng.integers(-8, 9, size=(k, n_rows))
        L4 = rng.integers(-8, 9, size=(k, n_rows))
        C4 = rng.integers(1, 9, size=(k, n_rows)) * rng.choice([-1, 1], size=(k, n_rows))
        self.W, self.Z, self.LAM, self.C = W4 / 4.0, Z4 / 4.0, L4 / 4.0, C4 / 4.0
        self.rho = np.array(MULTI_RHO[:k])
        v = (D8 @ W4.T).T * (UNIT // 32)
        res = Z4 * (UNIT // 4) - v
        lam1 = np.stack([L4[j] * (UNIT // 4) + _scale(res[j], float(self.rho[j])) for j in range(k)])
        self.ref = dict(v=_from_units(v), lam=_from_units(lam1),
                        primal2=[_sq_prefix(res[j], self.counts) for j in range(k)],
                        q={n: (D8[:n].T @ C4[:, :n].T).T / 32.0 for n in self.counts})
        assert np.array_equal(_to_units(self.ref["v"]), v) and np.array_equal(_to_units(self.ref["lam"]), lam1)
        fv = (self.D @ self.W.T).T
        fres = self.Z - fv
        self.f64 = dict(v=fv, lam=self.LAM + self.rho[:, None] * fres,
                        primal2=[{n: float(np.sum(fres[j, :n] ** 2)) for n in self.counts} for j in range(k)],
                        q={n: (self.D[:n].T @ self.C[:, :n].T).T for n in self.counts})

    def exactness_report(self):
        bad = [name for name in ("v", "lam") if not np.array_equal(self.ref[name], self.f64[name])]
        bad += [f"q[{n}]" for n in self.counts if not np.array_equal(self.ref["q"][n], self.f64["q"][n])]
        bad += [f"primal2[{j}][{n}]" for j in range(self.k) for n in self.counts
                if self.ref["primal2"][j][n] != self.f64["primal2"][j][n]]
        return bad


# ------------------------------------------------------------------------------------------------ real-valued inputs
REAL_RHO = (2e-7, 1e-3, 1.0)        # the values of test_prox_vs_oracle
REAL_SIGMA0 = 1e-2
DOT = 1e-13                          # x (absolute sum + 1): an fp64 dot product or column sum (test_gemv_gemvt)
ROOT = 1e-12                         # x max(1, |ref|): the prox root (test_prox_vs_oracle)
EPS = 2.0 ** -52


def _ulps(x):
    return 4.0 * EPS * np.abs(x)     # "a few ulps" of one rounded operation on operands of this size


class Real:
    """Standard normal inputs of one (storage, width, loss, rho), the reference and the propagated bounds.  Row-wise
    quantities for n_rows rows; q, primal2, zz and their bounds per n through sums(n)."""

    def __init__(self, storage, d, n_rows, loss, rho, seed):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.n, self.loss, self.rho = storage, d, n_rows, loss, rho
        self.rho_next, self.sigma0 = 1.02 * rho, REAL_SIGMA0
        self.D = storage_round(rng.standard_normal((n_rows, d)), storage)
        self.w, self.z_old, self.lam = rng.standard_normal(d), rng.standard_normal(n_rows), rng.standard_normal(n_rows)
        self.c_in = rng.standard_normal(n_rows)
        if loss == "binary_cross_entropy":          # the warm start of the root search: some far from the new root
            self.z_old[::5] += 40.0 * np.sign(self.z_old[::5])
        ext = np.longdouble
        self._Dx = self.D.astype(ext)
        A = np.abs(self.D)
        self._A = A
        v = np.asarray(self._Dx @ self.w.astype(ext), dtype=np.float64)
        res = self.z_old - v
        lam1 = self.lam + rho * res
        lr = lam1 / self.rho_next
        m = v - lr
        z = prox(loss, self.sigma0, self.rho_next, m) if loss else None
        self.ref = dict(v=v, lam=lam1, res=res)
        e_v = DOT * (A @ np.abs(self.w) + 1.0)
        e_res = e_v + _ulps(np.abs(self.z_old) + np.abs(v))
        e_lam = rho * e_v + _ulps(np.abs(self.lam) + rho * (np.abs(self.z_old) + np.abs(v)))
        self.err = dict(v=e_v, lam=e_lam, res=e_res)
        if z is not None:
            e_lr = e_lam / self.rho_next + _ulps(lr)
            e_m = e_v + e_lr + _ulps(np.abs(v) + np.abs(lr))
            self.ref.update(z=z, c=z + lr, lr=lr)
            self._e_lr, self._e_m = e_lr, e_m

    def sums(self, n):
        """reference and bounds of the n-row problem: the row-wise ones cut to n rows, the sums over them"""
        r, e = self.ref, self.err
        ref = dict(v=r["v"][:n], lam=r["lam"][:n], primal2=math.fsum((r["res"][:n] ** 2).tolist()))
        err = dict(v=e["v"][:n], lam=e["lam"][:n])
        err["primal2"] = float(np.sum(2.0 * np.abs(r["res"][:n]) * e["res"][:n] + e["res"][:n] ** 2)) + DOT * (ref["primal2"] + 1.0)
        if "z" in r:
            z, c = r["z"][:n], r["c"][:n]
            e_z = self._e_m[:n] + ROOT * max(1.0, float(np.max(np.abs(z))))     # the prox is 1-Lipschitz in m
            e_c = e_z + self._e_lr[:n] + _ulps(np.abs(z) + np.abs(r["lr"][:n]))
            A = self._A[:n]
            ref.update(z=z, c=c, q=np.asarray(self._Dx[:n].T @ c.astype(np.longdouble), dtype=np.float64),
                       zz=math.fsum((z ** 2).tolist()))
            err.update(z=e_z, q=A.T @ e_c + DOT * (A.T @ np.abs(c) + 1.0))
            err["zz"] = float(np.sum(2.0 * np.abs(z) * e_z + e_z ** 2)) + DOT * (ref["zz"] + 1.0)
        return ref, err

    def q_only(self, n):
        """q = D^T c_in of the first n rows and its bound"""
        c = self.c_in[:n]
        return (np.asarray(self._Dx[:n].T @ c.astype(np.longdouble), dtype=np.float64),
                DOT * (self._A[:n].T @ np.abs(c) + 1.0))


# ------------------------------------------------------------------------------------------------ the cases
def cases(pass_):
    """[(storage, instance)] of a pass: every instance of the table"""
    return [(st, inst) for st in STORAGES for inst in TABLE[pass_][st]]


def case_id(case):
    st, inst = case
    return f"{st}-{inst.kind}{inst.p}x{inst.r}x{inst.s}"


def all_counts(pass_, inst):
    """every row count a case runs, over both grids"""
    return sorted(set(row_counts(pass_, inst, 1)) | set(row_counts(pass_, inst, 2)))


def dyadic(pass_, storage, inst, d):
    """the dyadic fixture of one width (the V-only and Q-only passes share theirs, and so do the two multi-column ones)"""
    fam = "half" if pass_ in ("v", "q") else ("multi" if pass_.startswith("multi") else pass_)
    counts, seed = all_counts(pass_, inst), seed_of(fam, storage, d)
    cls = DyadicMulti if fam == "multi" else Dyadic
    return cls(storage, d, max(counts), counts, seed)


def rho_of(pass_, case, i):
    """the rho of width i of a case's real-valued inputs: every case runs all three over its three widths"""
    return REAL_RHO[(cases(pass_).index(case) + i) % len(REAL_RHO)]


def real(pass_, storage, inst, d, loss, rho):
    """the real-valued fixture of one width of the fused (one per loss), V-only or Q-only pass"""
    key = (pass_, storage, d, loss) if pass_ == "fused" else (pass_, storage, d)
    return Real(storage, d, n_max(pass_, inst), loss if pass_ == "fused" else None, rho, seed_of(*key))


def real_multi(pass_, storage, inst, d):
    """real-valued inputs of the multi-column passes, 4 columns: (D, W, Z, LAM, C)"""
    n = n_max(pass_, inst)
    rng = np.random.default_rng(seed_of(pass_, storage, d))
    D = storage_round(rng.standard_normal((n, d)), storage)
    return (D, rng.standard_normal((4, d)), rng.standard_normal((4, n)), rng.standard_normal((4, n)),
            rng.standard_normal((4, n)))


def seed_of(*key):
    """a reproducible seed from the case's parameters"""
    h = 0
    for part in key:
        for ch in str(part):
            h = (h * 131 + ord(ch)) % 1000003
    return h
