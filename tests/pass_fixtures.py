"""Reference, inputs and instance tables for the plain passes (csrc/sweep.hip: k_gemv, k_gemvt and its column-statistics
variant, k_colreduce) and the Gram kernels (csrc/gram.hip: k_gram, k_gram_reduce), run through the rbl_k_pass_* /
rbl_k_gram_full entry points with a chosen grid (a helper, not a conftest).

Tables: which kernel instance the launchers pick per range of 16-byte packets per row, restated as data (gemv_T /
gemv_dispatch, gemvt_T / gemvt_dispatch); the GPU tests assert that the instance a call reports is the table's.
Geometry: the launchers' grids restated as functions (gemv_dispatch's grid, gemvt_blocks and k_gemvt's rows_per_block,
gram_plan), from which the row counts are chosen so that a wave / a block runs its loop one, two and three times.

Two families of inputs, as in sweep_fixtures:
  dyadic       D in k/8, vectors in multiples of 1/4: every sum is exact in 53 bits in ANY order, so the device must
               return the reference's bits.  |k| <= 16; where a row has fewer than 4 columns, and in the first row of the
               Gram inputs, |k| <= 1024 (still exact in fp16), because 33 values cannot make rows / columns differ.
               The reference is computed in integers and in float64, and both must agree.
  real-valued  standard normal, D rounded to the storage type first; reference in extended precision; bounds from the
               project's constant DOT = 1e-13 x (absolute sum + 1) (test_gemv_gemvt) and u(x) = 4 x 2^-52 |x|:
                   e_v     = DOT (|D| |w| + 1)
                   e_q     = DOT (|D|^T |c| + 1)
                   e_sum   = DOT (sum |x| + 1)
                   e_sumsq = DOT (sum x^2 + 1) + sum u(x^2)            (the squares are rounded before they are added)
                   Gram    : 1e-12 n absolute, the bound of test_gram_mfma
"""
from collections import namedtuple

import numpy as np

from sweep_fixtures import DOT, PACKET, PAD, STORAGES, _ulps, any_order_exact, packets, seed_of, storage_round

LDS_ATTR_BYTES = 64 * 1024           # above it gemv_dispatch raises the kernel's dynamic LDS limit first
LDS_REFUSE_BYTES = 150 * 1024        # above it launch_gemv refuses the width
GEMVT_BLOCKS_PER_CU = 4              # RBL_GEMVT_BPC
GEMVT_MIN_ROWS = 64                  # gemvt_blocks: at least 64 rows per block
GT = 128                             # gram.hip: block tile


def pk_max(storage, ld_bytes):
    """the most packets per row whose w (ld doubles) fits ld_bytes"""
    return (ld_bytes // 8) // PACKET[storage]


# ------------------------------------------------------------------------------------------------ v = D w: the table
GemvInst = namedtuple("GemvInst", "pk_lo pk_hi lpr p u tag")   # tag: "" | "lds" (P = 0) | "lds_attr" (P = 0 above 64 KiB)


def _gemv_table(storage):
    t = [GemvInst(1, 1, 1, 1, 4, ""), GemvInst(2, 2, 2, 1, 4, ""), GemvInst(3, 4, 4, 1, 4, ""), GemvInst(5, 8, 8, 1, 4, ""),
         GemvInst(9, 16, 16, 1, 4, ""), GemvInst(17, 32, 32, 1, 4, ""), GemvInst(33, 64, 64, 1, 4, ""),
         GemvInst(65, 128, 64, 2, 4, ""), GemvInst(129, 256, 64, 4, 2, ""), GemvInst(257, 512, 64, 8, 1, ""),
         GemvInst(513, pk_max(storage, LDS_ATTR_BYTES), 64, 0, 4, "lds"),
         GemvInst(pk_max(storage, LDS_ATTR_BYTES) + 1, pk_max(storage, LDS_REFUSE_BYTES), 64, 0, 4, "lds_attr")]
    return t[1:] if storage == "f64" else t       # f64: ld % 4 == 0 makes the packet count even, never 1


GEMV_TABLE = {st: _gemv_table(st) for st in STORAGES}

# ------------------------------------------------------------------------------------------------ q = D^T c: the table
GemvtInst = namedtuple("GemvtInst", "pk_lo pk_hi tpr pj u tiles")
MAX_TILES = 3                        # the tables stop after three column tiles or at launch_gemv's refusal width


def _gemvt_table(storage):
    t = [GemvtInst(1, 1, 1, 1, 8, 1), GemvtInst(2, 2, 2, 1, 8, 1), GemvtInst(3, 4, 4, 1, 8, 1), GemvtInst(5, 8, 8, 1, 8, 1),
         GemvtInst(9, 16, 16, 1, 8, 1), GemvtInst(17, 32, 32, 1, 8, 1), GemvtInst(33, 64, 64, 1, 8, 1),
         GemvtInst(65, 128, 128, 1, 8, 1), GemvtInst(129, 256, 256, 1, 8, 1), GemvtInst(257, 512, 256, 2, 4, 1),
         GemvtInst(513, 1024, 256, 4, 2, 1)]
    end = pk_max(storage, LDS_REFUSE_BYTES)
    for tiles in range(1, MAX_TILES + 1):
        lo, hi = (1025 if tiles == 1 else 2048 * (tiles - 1) + 1), min(2048 * tiles, end)
        if lo <= hi:
            t.append(GemvtInst(lo, hi, 256, 8, 1, tiles))
    return t[1:] if storage == "f64" else t


COLSTATS_STORAGES = ("f32", "f64")   # launch_colstats refuses fp16
COLSTATS_TABLE = {st: _gemvt_table(st) for st in COLSTATS_STORAGES}
SWEEP_Q = (33, 512)                  # packets per row at which launch_gemvt hands the pass to launch_sweep_q
GEMVT_TABLE = {st: [i for i in _gemvt_table(st) if not (SWEEP_Q[0] <= i.pk_lo and i.pk_hi <= SWEEP_Q[1])] for st in STORAGES}
# the k_gemvt<T, TPR, PJ, U, SQ = false> instantiations no call of launch_gemvt reaches (T = float, double, rbl_half)
UNREACHABLE_GEMVT = [(64, 1, 8), (128, 1, 8), (256, 1, 8), (256, 2, 4)]
TABLES = {"v": GEMV_TABLE, "q": GEMVT_TABLE, "colstats": COLSTATS_TABLE}


def lookup(pass_, storage, d):
    pk = packets(d, storage)
    for inst in TABLES[pass_][storage]:
        if inst.pk_lo <= pk <= inst.pk_hi:
            return inst
    return None


def refused_width(storage):
    """the narrowest d launch_gemv refuses"""
    return pk_max(storage, LDS_REFUSE_BYTES) * PACKET[storage] + 1


def widths(storage, inst):
    """the narrowest and the widest d that select the instance and one with padded columns below the widest (the
    narrowest is padded too).  P = 0: also a width whose packet count is a multiple of 256 (no tail loop after the
    4-pass blocks) and a padded one two packets wider."""
    e, pad = PACKET[storage], PAD[storage]
    ld_min = -(-inst.pk_lo * e // pad) * pad
    d_max = inst.pk_hi * e
    w = {ld_min - pad + 1, d_max - 1, d_max}
    if getattr(inst, "p", 1) == 0:
        m = -(-inst.pk_lo // 256) * 256
        assert m <= inst.pk_hi
        w |= {m * e, (m + 2) * e - 1}
        assert (m + 2) <= inst.pk_hi
    return tuple(sorted(x for x in w if x >= 1))


# ------------------------------------------------------------------------------------------------ v = D w: the grid
def gemv_grid(inst, num_cu, n):
    """blocks gemv_dispatch launches"""
    rpw = 64 // inst.lpr
    need = -(-n // (4 * rpw * 2))
    return max(1, min(num_cu * 8, need))


def gemv_reported(inst, num_cu, n):
    return (inst.lpr, inst.p, inst.u, gemv_grid(inst, num_cu, n))


def gemv_stride(inst, num_cu, n):
    """rows between two steps of one wave: GW x RS"""
    return 4 * gemv_grid(inst, num_cu, n) * (64 // inst.lpr) * inst.u


def gemv_steps(inst, num_cu, n):
    """steps of the busiest wave (wave 0 of block 0)"""
    rs = (64 // inst.lpr) * inst.u
    return -(-(-(-n // rs)) // (4 * gemv_grid(inst, num_cu, n)))


def gemv_one_step_rows(inst, num_cu):
    """the largest n at which no wave runs its loop twice.  U >= 2: every wave of the full grid has one step.  U = 1
    (P = 8): the grid is sized for 8 rows per block and a block's step covers 4, so only one block's 4 rows qualify."""
    rs = (64 // inst.lpr) * inst.u
    return 32 * num_cu * rs if inst.u >= 2 else 4 * rs


def gemv_row_counts(inst, num_cu):
    """a single row; a tail in the second lane group; around one step of a wave; every wave exactly one step, and one
    row more; the third round with a ragged last step whose second lane group is ragged too"""
    rpw = 64 // inst.lpr
    rs = rpw * inst.u
    one = gemv_one_step_rows(inst, num_cu)
    third = 2 * 32 * num_cu * rs + rs + rpw + 1
    return sorted({1, rpw + 1, rs - 1, rs, rs + 1, one, one + 1, third} - {0})


# ------------------------------------------------------------------------------------------------ q = D^T c: the grid
def gemvt_nb(num_cu, n):
    """gemvt_blocks: row blocks = slab rows k_colreduce adds"""
    return max(1, min(num_cu * GEMVT_BLOCKS_PER_CU, -(-n // GEMVT_MIN_ROWS)))


def gemvt_rows_per_block(num_cu, n):
    return -(-n // gemvt_nb(num_cu, n))


def gemvt_reported(inst, num_cu, n):
    return (inst.tpr, inst.pj, inst.u, gemvt_nb(num_cu, n), inst.tiles)


def gemvt_steps(inst, num_cu, n):
    """steps of the busiest block (block 0)"""
    return -(-gemvt_rows_per_block(num_cu, n) // ((256 // inst.tpr) * inst.u))


def gemvt_one_step_rows(inst, num_cu):
    """the largest n at which no block runs its loop twice: every block of the full grid one step - or, where a step
    is shorter than the 64 rows a block gets at least, the single block's one step"""
    s = (256 // inst.tpr) * inst.u
    return num_cu * GEMVT_BLOCKS_PER_CU * s if s >= GEMVT_MIN_ROWS else s


def gemvt_third_step_rows(inst, num_cu):
    """the full grid, every block in its third step or later, the last step with a ragged second row group: two steps
    (at least the 64 rows that keep the grid full) and RPB + 1 rows more per block, less one row in the last block"""
    rpb = 256 // inst.tpr
    s = rpb * inst.u
    extra = rpb + 1 if (rpb + 1) % s else 1          # (one packet per thread and two rows in flight: RPB + 1 = S)
    return num_cu * GEMVT_BLOCKS_PER_CU * (max(2 * s, GEMVT_MIN_ROWS) + extra) - 1


def gemvt_row_counts(inst, num_cu):
    """a single row; around one step; every block exactly one step, and one row more; the third step with ragged row
    groups (and a ragged last block); the fewest rows that fill the grid, which are no multiple of the block count"""
    rpb = 256 // inst.tpr
    s = rpb * inst.u
    nb = num_cu * GEMVT_BLOCKS_PER_CU
    one = gemvt_one_step_rows(inst, num_cu)
    third = gemvt_third_step_rows(inst, num_cu)
    full = GEMVT_MIN_ROWS * (nb - 1) + 1
    return sorted({1, s - 1, s, s + 1, one, one + 1, third, full} - {0})


MANY_BLOCKS = (5, 20 * GEMVT_MIN_ROWS + 37)    # (num_cu, n): 20 slab rows, more than the 16 row groups of k_colreduce


def gemvt_grids(inst):
    """[(num_cu, n)] of an instance; up to 32 packets per row also the grid with more than 16 slab rows"""
    g = [(cu, n) for cu in (1, 2) for n in gemvt_row_counts(inst, cu)]
    return g + [MANY_BLOCKS] if inst.pk_hi <= 32 else g


def empty_tail_rows(cus):
    """n at which all 4 x cus blocks are launched and the last one has no rows ((nb - 1) x rows_per_block >= n), or None
    where the device is too small for one (65 rows per block need more than 65 blocks)"""
    nb = cus * GEMVT_BLOCKS_PER_CU
    n = (nb - 1) * (GEMVT_MIN_ROWS + 1)
    ok = gemvt_nb(cus, n) == nb and (nb - 1) * gemvt_rows_per_block(cus, n) >= n
    return n if ok else None


# ------------------------------------------------------------------------------------------------ G = D^T D: the plan
GRAM_WIDTHS = (1, 127, 128, 129, 256, 257)
GRAM_SINGLE_ROW_SPLIT = 57          # 8 splits of 8 rows: the last one holds row 56 alone
GRAM_EMPTY_SPLITS = 9               # 8 splits of 8 rows: one full, one with a single row, six without rows
GRAM_ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 2048, 2049, GRAM_SINGLE_ROW_SPLIT, GRAM_EMPTY_SPLITS)


def gram_plan(ld, n, num_cu):
    """(ntiles, npairs, ksplit, rows_per_split) as gram.hip's gram_plan computes them"""
    ntiles = -(-ld // GT)
    npairs = ntiles * (ntiles + 1) // 2
    want = max(1, min(-(-num_cu * 4 // npairs), -(-n // 256)))
    want = -(-want // 8) * 8
    rps = max(8, -(-(-(-n // want)) // 8) * 8)
    return (ntiles, npairs, want, rps)


# ------------------------------------------------------------------------------------------------ dyadic inputs
def _k_max(d):
    return 16 if d >= 4 else 1024


class DyadicPass:
    """D (n_rows x d) in k/8, w and c in multiples of 1/4; v for every row, q / sum / sumsq per n in counts.
    offsets: row distances at which v must differ (rows one lane group handles in one step, rows one wave handles in
    consecutive rounds)."""

    def __init__(self, storage, d, n_rows, counts, offsets, seed, sums=True):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.n, self.counts = storage, d, n_rows, tuple(sorted(counts))
        self.sums = sums                                           # False: v alone (the v pass' fixtures)
        self.offsets = tuple(sorted(o for o in set(offsets) if 0 < o < n_rows))
        km = _k_max(d)
        D8 = rng.integers(-km, km + 1, size=(n_rows, d))
        w4 = rng.integers(-4, 5, size=d)
        w4[0] = 1                                                  # a unit step of D[i, 0] moves v[i]
        c4 = rng.integers(1, 9, size=n_rows) * rng.choice([-1, 1], size=n_rows)    # never 0
        for _ in range(200):
            v32 = D8 @ w4
            bad = ~np.any(D8 != 0, axis=1)
            for o in self.offsets:
                bad[o:] |= v32[o:] == v32[:-o]
            if not bad.any():
                break
            D8[bad] = rng.integers(-km, km + 1, size=(int(bad.sum()), d))
        else:
            raise AssertionError("no dyadic D with distinct v at the given offsets")
        self.D8, self.w4, self.c4 = D8, w4, c4
        self.D, self.w, self.c = D8 / 8.0, w4 / 4.0, c4 / 4.0
        assert np.array_equal(storage_round(self.D, storage), self.D)
        A = np.abs(D8)
        assert any_order_exact(int(np.max(A @ np.abs(w4))), [1])
        self.i_v = v32                                             # units of 1/32
        self.ref, self.f64 = dict(v=v32 / 32.0), dict(v=self.D @ self.w)
        if not sums:
            return
        pre_q, pre_s, pre_s2, pre_aq, pre_a, pre_a2 = (_prefix(x, self.counts) for x in (
            D8 * c4[:, None], D8, D8 * D8, A * np.abs(c4)[:, None], A, A * A))
        for pre in (pre_aq, pre_a, pre_a2):                        # the absolute sums bound every partial sum
            assert any_order_exact(int(max(np.max(x) for x in pre.values())), [1]), "a sum does not fit 53 bits"
        self.i_q, self.i_sum, self.i_sumsq = pre_q, pre_s, pre_s2  # units of 1/32, 1/8, 1/64
        self.ref.update(q={n: pre_q[n] / 32.0 for n in self.counts}, sum={n: pre_s[n] / 8.0 for n in self.counts},
                        sumsq={n: pre_s2[n] / 64.0 for n in self.counts})
        self.f64.update(q={n: self.D[:n].T @ self.c[:n] for n in self.counts},
                        sum={n: self.D[:n].sum(axis=0) for n in self.counts},
                        sumsq={n: (self.D[:n] ** 2).sum(axis=0) for n in self.counts})

    def exactness_report(self):
        bad = [] if np.array_equal(self.ref["v"], self.f64["v"]) else ["v"]
        for name in (("q", "sum", "sumsq") if self.sums else ()):
            bad += [f"{name}[{n}]" for n in self.counts if not np.array_equal(self.ref[name][n], self.f64[name][n])]
        return bad


class DyadicGram:
    """D in k/8 with pairwise different columns: the first row holds d different non-zero values (|k| <= 1024), so the
    columns differ at every row count; G per n in counts, in integers (units of 1/64) and in float64"""

    def __init__(self, storage, d, counts, seed):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.counts = storage, d, tuple(sorted(counts))
        self.n = n = max(counts)
        D8 = rng.integers(-16, 17, size=(n, d))
        vals = np.concatenate([np.arange(-1024, 0), np.arange(1, 1025)])
        D8[0] = rng.choice(vals, size=d, replace=False)
        zero = ~np.any(D8 != 0, axis=1)
        D8[zero, 0] = 1
        self.D8, self.D = D8, D8 / 8.0
        assert np.array_equal(storage_round(self.D, storage), self.D)
        A = np.abs(D8)
        assert any_order_exact(int(np.max(A.T @ A)), [1])
        self.i_G, acc, i = {}, np.zeros((d, d), dtype=np.int64), 0
        for m in self.counts:
            acc = acc + D8[i:m].T @ D8[i:m]
            self.i_G[m], i = acc, m
        self.ref = {m: self.i_G[m] / 64.0 for m in self.counts}

    def f64(self, m):
        return self.D[:m].T @ self.D[:m]


# ------------------------------------------------------------------------------------------------ real-valued inputs
def _prefix(terms, counts):
    """column sums of the first n rows, per n in counts"""
    out, acc, i = {}, np.zeros(terms.shape[1:], dtype=terms.dtype), 0
    for n in sorted(counts):
        acc = acc + terms[i:n].sum(axis=0)
        out[n], i = acc, n
    return out


def _prefix_ext(terms, counts):
    """column sums of the first n rows in extended precision, per n in counts -> float64"""
    out, acc, i = {}, np.zeros(terms.shape[1:], dtype=np.longdouble), 0
    for n in sorted(counts):
        acc = acc + terms[i:n].sum(axis=0, dtype=np.longdouble)
        out[n], i = np.asarray(acc, dtype=np.float64), n
    return out


class RealPass:
    """standard normal D (rounded to the storage type), w, c; references in extended precision and the bounds"""

    def __init__(self, storage, d, n_rows, counts, seed, sums=True):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.n, self.counts = storage, d, n_rows, tuple(sorted(counts))
        self.D = storage_round(rng.standard_normal((n_rows, d)), storage)
        self.w, self.c = rng.standard_normal(d), rng.standard_normal(n_rows)
        A = np.abs(self.D)
        Dx = self.D.astype(np.longdouble)
        self.v = np.asarray(Dx @ self.w.astype(np.longdouble), dtype=np.float64)
        self.e_v = DOT * (A @ np.abs(self.w) + 1.0)
        if not sums:
            return
        cx = self.c.astype(np.longdouble)[:, None]
        self.q = _prefix_ext(Dx * cx, counts)
        self.sum = _prefix_ext(Dx, counts)
        self.sumsq = _prefix_ext(Dx * Dx, counts)
        aq, a1, a2 = (_prefix(x, counts) for x in (A * np.abs(self.c)[:, None], A, A * A))   # (bounds: float64 will do)
        self.e_q = {n: DOT * (aq[n] + 1.0) for n in counts}
        self.e_sum = {n: DOT * (a1[n] + 1.0) for n in counts}
        self.e_sumsq = {n: DOT * (a2[n] + 1.0) + _ulps(a2[n]) for n in counts}    # sum u(x^2) = u(sum x^2)


class RealGram:
    def __init__(self, storage, d, counts, seed):
        rng = np.random.default_rng(seed)
        self.storage, self.d, self.counts = storage, d, tuple(sorted(counts))
        self.n = max(counts)
        self.D = storage_round(rng.standard_normal((self.n, d)), storage)
        Dx, A = self.D.astype(np.longdouble), np.abs(self.D)
        self.G, self.scale = {}, {}
        acc, acc_a, i = np.zeros((d, d), dtype=np.longdouble), np.zeros((d, d)), 0
        for m in self.counts:
            acc = acc + np.einsum("ki,kj->ij", Dx[i:m], Dx[i:m])     # (several times faster than @ on extended precision)
            acc_a = acc_a + A[i:m].T @ A[i:m]
            self.G[m], self.scale[m], i = np.asarray(acc, dtype=np.float64), DOT * (acc_a + 1.0), m


GRAM_REAL_ROWS = (1, 5, 17, 65, GRAM_SINGLE_ROW_SPLIT, 2049)   # the extended-precision reference costs n d^2 slow flops


# ------------------------------------------------------------------------------------------------ the cases
def cases(pass_):
    return [(st, inst) for st in TABLES[pass_] for inst in TABLES[pass_][st]]


def case_id(case):
    st, inst = case
    if isinstance(inst, GemvInst):
        return f"{st}-lpr{inst.lpr}p{inst.p}u{inst.u}{inst.tag}"
    return f"{st}-tpr{inst.tpr}pj{inst.pj}u{inst.u}t{inst.tiles}"


def gram_cases():
    return [(st, d) for st in STORAGES for d in GRAM_WIDTHS]


def gemv_counts(inst):
    return sorted(set(gemv_row_counts(inst, 1)) | set(gemv_row_counts(inst, 2)))


def gemv_offsets(inst):
    """row distances at which v_ref must differ: r + u x RPW inside a step, r + stride for every grid a case runs"""
    rpw = 64 // inst.lpr
    return sorted({u * rpw for u in range(1, inst.u)} | {gemv_stride(inst, cu, n) for cu in (1, 2) for n in gemv_row_counts(inst, cu)})


def gemvt_counts(inst):
    return sorted({n for _, n in gemvt_grids(inst)})


def dyadic_v(storage, inst, d):
    counts = gemv_counts(inst)
    return DyadicPass(storage, d, max(counts), counts, gemv_offsets(inst), seed_of("pass_v", storage, d), sums=False)


def real_v(storage, inst, d):
    counts = gemv_counts(inst)
    return RealPass(storage, d, max(counts), counts, seed_of("pass_v_real", storage, d), sums=False)


def dyadic_q(storage, inst, d):
    """the fixture of the q pass and of colstats at one width"""
    counts = gemvt_counts(inst)
    return DyadicPass(storage, d, max(counts), counts, (), seed_of("pass_q", storage, d))


def real_q(storage, inst, d):
    counts = gemvt_counts(inst)
    return RealPass(storage, d, max(counts), counts, seed_of("pass_q_real", storage, d))


def dyadic_gram(storage, d):
    return DyadicGram(storage, d, GRAM_ROWS, seed_of("gram", storage, d))


def real_gram(storage, d):
    return RealGram(storage, d, GRAM_REAL_ROWS, seed_of("gram_real", storage, d))
