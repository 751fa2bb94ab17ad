"""The z-step's 32-bit sort keys, restated (csrc/elementwise.hip: k_make_m_range, k_keys32, k_sort32_fix).

keys32 repeats the device's operations in the device's order; librbl is built with -ffp-contract=off, so IEEE
double arithmetic gives the device's keys bit for bit.  Test infrastructure only - see oracle/__init__.py.
NaN in m is not covered: a solve produces one only after it has diverged.
"""
import numpy as np

MAX_RUN = 32          # S32_MAX_RUN: the longest run of equal keys the fix-up repairs; a longer one raises the flag
KEY_MAX = 4294967295.0


def keys32(m):
    """uint32 keys of m: the fixed-point image on [min m, max m].  scale = 4294967295 / (hi - lo); a range that is
    empty, not finite, or so small that the scale overflows is degenerate (scale 0: every key 0); the product is
    truncated towards zero and saturates at 0xffffffff; what is not > 0 (a NaN from inf * 0 included) is key 0."""
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    if m.size == 0:
        return np.zeros(0, dtype=np.uint32)
    lo, hi = m.min(), m.max()
    with np.errstate(all="ignore"):
        scale = np.float64(KEY_MAX) / (hi - lo)
        if not (hi > lo) or not (scale < 1.7e308):
            scale = np.float64(0.0)
        t = (m - lo) * scale
        inside = (t > 0.0) & (t < KEY_MAX)
        keys = np.where(inside, t, 0.0).astype(np.uint64).astype(np.uint32)    # (u32) t: truncation
        keys[t >= KEY_MAX] = 0xFFFFFFFF
    return keys


def max_run(keys):
    """length of the longest run of equal keys once they are sorted"""
    keys = np.asarray(keys)
    if keys.size == 0:
        return 0
    k = np.sort(keys, kind="stable")
    edges = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1], [True])))
    return int(np.diff(edges).max())


def flagged(m):
    """does the fix-up raise its flag on m (a run longer than MAX_RUN)?"""
    return max_run(keys32(m)) > MAX_RUN


def min_gap_in_keys(m):
    """the smallest distance between two DIFFERENT values of m, in units of the key spacing (range / 2^32): values
    further apart than a few units cannot be pushed into one key by rounding differences of ~1e-12 in m"""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    u = np.unique(m)
    if u.size < 2:
        return np.inf
    return float(np.diff(u).min() / ((u[-1] - u[0]) / 2.0 ** 32))


def expected(m, idx_off=0):
    """(order, m_sorted, ids) of the (m, row) order: np.argsort(m, kind="stable") - a numerical comparison, so -0.0 and
    +0.0 tie and keep their row order -, m[order] with the input's bits, and the row ids order + idx_off as uint32"""
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    order = np.argsort(m, kind="stable")
    ids = (order.astype(np.uint64) + np.uint64(idx_off)).astype(np.uint32)
    return order, m[order], ids
