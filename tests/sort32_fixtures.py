"""Inputs of the 32-bit-key sort tests (test_sort32_host.py pins what oracle/sort32.py says about each of them on a
CPU, test_gpu_sort32.py runs them on the device).  Every fixture draws from its own np.random.default_rng(2).

Length-critical fixtures are built from EXACT duplicates: equal m share a key whatever the rounding.  Clusters of near
ties (spacing 2^-45 of the range, the keys' spacing is 2^-32 of it) may straddle a key boundary and are only used where
a split is harmless: the bit-exact check of the (m, row) order holds either way."""
import functools

import numpy as np

SEED = 2
SIZES = (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 70001, 1 << 20)
DUP_MULTS = (2, 3, 31, 32, 33)
BOUNDARY_P = (240, 255, 4080, 4095)          # a run of 32 across sorted positions 256 and 4096
WRAP_N = 16384 * 256 + 4097                  # past the fix-up's 16384 blocks of 256 threads: its grid-stride loop wraps
MIXTURE_SIZES = (4097, 70001, 1 << 20)


def _rng():
    return np.random.default_rng(SEED)


def gaussian(n):
    return _rng().standard_normal(n)


def duplicates(mult, nbase=500):
    """one value `mult` times, shuffled among nbase distinct Gaussian rows"""
    rng = _rng()
    base = rng.standard_normal(nbase)
    v = rng.standard_normal()
    m = np.concatenate((base, np.full(mult, v)))
    return m[rng.permutation(m.size)]


def boundary(p, mult=32, nlarger=100):
    """a run of `mult` equal values with exactly p smaller rows (and nlarger larger ones), shuffled: the run occupies
    the sorted positions p ... p + mult - 1"""
    rng = _rng()
    m = np.concatenate((rng.uniform(-2.0, -1.0, p), np.full(mult, 0.25), rng.uniform(1.0, 2.0, nlarger)))
    return m[rng.permutation(m.size)]


def near_ties(sizes=(2, 3, 4, 5, 6, 7, 8), nbase=500):
    """clusters of 2 ... 8 values spaced 2^-45 of the range, each stored in DESCENDING m by row: the stable sort
    delivers a cluster that shares a key in row order, i.e. reversed, and the fix-up has to turn it round"""
    rng = _rng()
    base = rng.standard_normal(nbase)
    step = (base.max() - base.min()) * 2.0 ** -45
    parts = [base]
    for c, x in zip(sizes, np.linspace(-1.0, 1.0, len(sizes)) + 0.0123):
        parts.append(x + step * np.arange(c - 1, -1, -1))
    return np.concatenate(parts)


def mixed_run(nbase=500):
    """exact ties and near ties in one run: rank by m, then by row"""
    rng = _rng()
    base = rng.standard_normal(nbase)
    step = (base.max() - base.min()) * 2.0 ** -45
    x = 0.3021
    lv = np.array([2, 1, 1, 0, 2, 0, 1, 3, 0, 3, 2, 1])
    m = np.concatenate((base[:250], x + step * lv[:6], base[250:], x + step * lv[6:]))
    return m


def grid(n=20000):
    """m on a 2-decimal grid: long runs of exactly equal values"""
    return np.round(_rng().standard_normal(n), 2)


def mixture(n):
    """the key mixture of test_gpu_kernels.py::test_sort_bit_exact"""
    rng = _rng()
    return rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)


def wrap():
    """Gaussian rows past 16384 * 256, with a run of 32 near the top of the order: it is repaired by threads in their
    second trip of the grid-stride loop"""
    rng = _rng()
    m = rng.standard_normal(WRAP_N)
    m[rng.choice(WRAP_N, size=32, replace=False)] = 3.5
    return m


def ends(nbase=500):
    """several rows equal to min m (key 0) and to max m (the saturated key 0xffffffff): range 8, a power of two, so
    the scale and the image of the maximum are exact"""
    rng = _rng()
    m = np.clip(rng.standard_normal(nbase), -3.5, 3.5)
    m[rng.choice(nbase, size=9, replace=False)] = [4.0] * 5 + [-4.0] * 4
    return m


def signed_zeros():
    return np.array([0.0, -0.0, 1.0, -1.0, -0.0, 0.0, -0.0])


def band_edge_runs(n=4000, edges=(800, 3200), half=4):
    """distinct values with an exact-duplicate run of 2 * half placed across each of the given ranks (aorr [0.2, 0.8] at n = 4000:
    the weights change at ranks 800, 801 and 3200), rows shuffled"""
    rng = _rng()
    m = np.sort(rng.standard_normal(n))
    for e in edges:
        m[e - half:e + half] = m[e - half]
    return m[rng.permutation(n)]


def replicated_problem(times, n0=100, d=8, seed=SEED):
    """a data set in which every row (and its label) appears `times` times, copies interleaved"""
    from oracle import problems
    X0, y0 = problems.make_problem(n0, d, seed=seed)
    return np.tile(X0, (times, 1)), np.tile(np.asarray(y0, dtype=np.float64).reshape(-1), times)


# name -> (builder, built from exact duplicates?, has signed zeros?)
_F = {}


def _add(name, fn, exact=False, zeros=False):
    _F[name] = (fn, exact, zeros)


for _n in SIZES:
    _add(f"gauss_{_n}", functools.partial(gaussian, _n))
for _k in DUP_MULTS:
    _add(f"dup_x{_k}", functools.partial(duplicates, _k), exact=True)
for _p in BOUNDARY_P:
    _add(f"run32_after_{_p}", functools.partial(boundary, _p), exact=True)
_add("run33_after_4080", functools.partial(boundary, 4080, 33), exact=True)
_add("near_ties", near_ties)
_add("cluster8", functools.partial(near_ties, (8,)))
_add("mixed_run", mixed_run)
_add("grid_20000", grid, exact=True)
for _n in MIXTURE_SIZES:
    _add(f"mixture_{_n}", functools.partial(mixture, _n))
_add("wrap", wrap, exact=True)
_add("all_equal_32", lambda: np.full(32, 0.7), exact=True)
_add("all_equal_33", lambda: np.full(33, 0.7), exact=True)
_add("overflow_12", lambda: np.array([1e308, -1e308] + [0.0] * 10), exact=True)
_add("overflow_42", lambda: np.array([1e308, -1e308] + [0.0] * 40), exact=True)
_add("inf_22", lambda: np.concatenate(([np.inf, -np.inf], gaussian(20))))
_add("inf_plus_only_22", lambda: np.concatenate(([np.inf], gaussian(21))))
_add("inf_300", lambda: np.concatenate(([np.inf, -np.inf], gaussian(298))))
_add("range_1e-290", lambda: 1e-290 * _rng().random(300))
_add("denormal_20", lambda: 5e-324 * _rng().permutation(20))
_add("denormal_40", lambda: 5e-324 * _rng().permutation(40))
_add("ends", ends, exact=True)
_add("signed_zeros", signed_zeros, exact=True, zeros=True)
_add("band_edge_runs", band_edge_runs, exact=True)

NAMES = tuple(_F)


@functools.lru_cache(maxsize=None)
def get(name):
    """the fixture's m (read-only; built once per process)"""
    m = np.ascontiguousarray(_F[name][0](), dtype=np.float64)
    m.setflags(write=False)
    return m


def exact(name):
    return _F[name][1]


def has_signed_zeros(name):
    return _F[name][2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(longest run, flag, order, m_sorted, ids at idx_off = 0) by oracle/sort32.py, computed once"""
    from oracle import sort32
    m = get(name)
    run = sort32.max_run(sort32.keys32(m))
    order, ms, ids = sort32.expected(m, 0)
    for a in (order, ms, ids):
        a.setflags(write=False)
    return run, int(run > sort32.MAX_RUN), order, ms, ids


REPLICATED_CASES = {
    "extremile_bce_l1": dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
    "esrm_hinge_l2": dict(weight_function="esrm", loss="hinge", l2_reg=0.01, args=[1.0]),
}
IDENTITY_CASES = dict(REPLICATED_CASES,
                      ehrm_bce_l2=dict(weight_function="ehrm", loss="binary_cross_entropy", l2_reg=0.01, B=-5))


def gaussian_problem():
    """the Gaussian data of the comparison of the 32-bit and the 64-bit keys"""
    from oracle import problems
    X, y = problems.make_problem(3000, 8, seed=6)
    return X, np.asarray(y, dtype=np.float64).reshape(-1)


def oracle_m(X, y, kw, k):
    """m = D w - lambda / rho that iteration k (k >= 1) of the CPU oracle's exact solve starts from"""
    from oracle import admm
    r = admm.admm_solve(X, y, max_iter=k, mode="exact", tol=0.0, store=False, **kw)
    D = -np.asarray(y, dtype=np.float64).reshape(-1, 1) * X
    return D @ r.w - r.lam / r.rho_final
