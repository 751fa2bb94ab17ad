"""NumPy restatement of the column statistic of scale-only standardisation on sparse storage (include/rbl.h:
rbl_set_centering; csrc/spmv.hip: k_csc_stat_segments, k_csc_columns), in the kernels' summation order, so that the vectors
of RBL_SCALE_FIT on a handle with RBL_STORE_CSR can be compared in bits.

A column with cnt stored entries of n (explicit zeros are stored entries), its source values x in ascending row order:

    sh  = x[0] if cnt == n else 0            (the shift of the dense statistics: a full constant column sums exact zeros)
    m   = sum (x - sh) / n
    var = (sum ((x - sh) - m)^2 + (n - cnt) m^2) / n,     scale = sqrt(var), or 1 where var is not > 0

Each of the two sums is two-stage.  The entry list is cut into segments of SEG entries; within a segment lane l of 64 adds
the entries 2l, 2l + 1, 2l + 128, 2l + 129, ... in that order (plain adds, no fused multiply-add), then the lanes are folded
by a butterfly (a[l] += a[l ^ off], off = 32 .. 1).  The segments' sums of a column are added by 16 lanes - lane l takes the
segments l, l + 16, ... in order - and folded by the same butterfly (off = 8 .. 1).

map_point: the point (w, b) of the fully standardised model, x_std . w + b with x_std = (x - mean) / scale, in the
scale-only model: x_scaled . w + (b - sum_j w_j mean_j / scale_j)."""
import numpy as np

SEG = 2048          # RBL_CSC_SEG (csrc/csc_plan.h)
WAVE = 64
FOLD_LANES = 16     # SP_QL (csrc/spmv.hip)


def _butterfly(a):
    idx = np.arange(a.size)
    off = a.size // 2
    while off >= 1:
        a = a + a[idx ^ off]
        off //= 2
    return a[0]


def segment_sum(t):
    """one wave's sum of the terms t of a segment (t.size <= SEG), in entry order"""
    t = np.asarray(t, dtype=np.float64)
    step = 2 * WAVE
    padded = np.zeros(-(-max(t.size, 1) // step) * step)      # (acc + 0.0 leaves acc's bits: acc is never -0.0)
    padded[:t.size] = t
    acc = np.zeros(WAVE)
    for blk in padded.reshape(-1, WAVE, 2):
        acc = acc + blk[:, 0]
        acc = acc + blk[:, 1]
    return _butterfly(acc)


def column_sum(t, seg=SEG):
    """the two-stage sum of a column's terms t (entry order)"""
    t = np.asarray(t, dtype=np.float64)
    parts = np.array([segment_sum(t[a:a + seg]) for a in range(0, t.size, seg)], dtype=np.float64)
    acc = np.zeros(FOLD_LANES)
    for l in range(FOLD_LANES):
        for p in parts[l::FOLD_LANES]:
            acc[l] = acc[l] + p
    return _butterfly(acc)


def column_stat(x, n, seg=SEG):
    """x: the column's stored source values in ascending row order, n: rows -> dict with the shift, both term vectors and
    sums, the mean of the shifted values, the variance and the scale"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    cnt = x.size
    sh = x[0] if (cnt == n and cnt > 0) else 0.0
    dl = x - sh
    s1 = column_sum(dl, seg)
    m1 = s1 / float(n)
    t = dl - m1
    t = t * t
    s2 = column_sum(t, seg)
    var = (s2 + float(n - cnt) * (m1 * m1)) / float(n)
    scale = np.sqrt(var) if var > 0.0 else 1.0
    return dict(shift=sh, terms1=dl, s1=s1, m1=m1, terms2=t, s2=s2, mean=sh + m1, var=var, scale=float(scale), cnt=cnt)


def csr_columns(indptr, indices, data, ncols):
    """the stored values of every column of a canonical CSR matrix, in ascending row order (explicit zeros included)"""
    indices = np.asarray(indices).astype(np.int64)
    data = np.asarray(data).astype(np.float64)           # widening float32 / float16 is exact
    order = np.argsort(indices, kind="stable")           # stable: rows stay ascending within a column
    bounds = np.searchsorted(indices[order], np.arange(ncols + 1))
    return [data[order[bounds[j]:bounds[j + 1]]] for j in range(ncols)]


def fit_csr(A, seg=SEG):
    """(mean, scale) of the columns of the scipy.sparse CSR matrix A as RBL_SCALE_FIT with centring off computes the scale
    on sparse storage; the handle reports zeros for the mean - the true means are returned for map_point"""
    n, d = A.shape
    stats = [column_stat(x, n, seg) for x in csr_columns(A.indptr, A.indices, A.data, d)]
    return np.array([s["mean"] for s in stats]), np.array([s["scale"] for s in stats])


def map_point(w, b, mean, scale):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    return w.copy(), float(b) - float(np.sum(w * np.asarray(mean, dtype=np.float64) / np.asarray(scale, dtype=np.float64)))
