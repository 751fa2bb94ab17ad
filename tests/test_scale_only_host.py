"""Scale-only standardisation (include/rbl.h: rbl_set_centering; ``standardize="scale"``), the part that needs no GPU: the
two symbols in header, library and binding, the Python refusals before any device call, and the NumPy restatement of the
sparse column statistic (tests/scale_only_ref.py) - exact where every sum is exact, and within the textbook bound of a
k-term sum on real data."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

sp = pytest.importorskip("scipy.sparse")

import scale_only_ref as ref     # noqa: E402
import scaling_ref               # noqa: E402


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def test_symbols_are_declared_exported_and_bound():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    declared = set(re.findall(r"\b(rbl_[A-Za-z0-9_]+)\s*\(", header))
    lib = rbl._lib.load()
    for name in ("rbl_set_centering", "rbl_get_centering"):
        assert name in declared and name in rbl._lib.SIGNATURES and hasattr(lib, name), name
    assert "#define RBL_VERSION 106" in header and lib.rbl_version() == 106
    assert rbl._lib.SCALING == {"none": 0, "fit": 1, "apply": 2}          # the mode is handle state, not a scaling value


def _data(n=30, d=6):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.3)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return X, y


def test_unknown_standardize_string_is_refused_before_any_device_call():
    rbl = _pkg()
    X, y = _data()
    A = sp.csr_matrix(X)
    msg = r"standardize must be False, True or \"scale\", got 'maxabs'"
    for storage, M in (("f32", X), ("csr", A)):
        with pytest.raises(ValueError, match=msg):
            rbl.ADMMmethod(M, y, "erm", "binary_cross_entropy", l1_reg=0.01, storage=storage, standardize="maxabs")
        with pytest.raises(ValueError, match=msg):
            rbl.OneVsRest(M, np.arange(X.shape[0]) % 3, l2_reg=0.1, storage=storage, standardize="maxabs")
        with pytest.raises(ValueError, match="problem 0: " + msg):
            rbl.ADMMgroup(M, y, [dict(l2_reg=0.1, standardize="maxabs")], storage=storage)
    with pytest.raises(ValueError, match=msg):
        rbl.smoothADMMmethod(X, y, "erm", "hinge", l1_reg=0.01, standardize="maxabs")


def test_mixed_modes_in_a_group_are_refused_before_any_device_call():
    rbl = _pkg()
    X, y = _data()
    msg = "problem 1: standardize must be the same for every problem of a group"
    for a, b in ((True, "scale"), ("scale", True), ("scale", False), (False, "scale")):
        with pytest.raises(ValueError, match=msg):
            rbl.ADMMgroup(X, y, [dict(l2_reg=0.1, standardize=a), dict(l2_reg=0.2, standardize=b)])
    with pytest.raises(ValueError, match=msg):
        rbl.ADMMgroup(sp.csr_matrix(X), y, [dict(l2_reg=0.1, standardize="scale"), dict(l2_reg=0.2)], storage="csr")


def test_true_on_csr_keeps_its_refusal():
    rbl = _pkg()
    X, y = _data()
    A = sp.csr_matrix(X)
    old = r'standardize=True with storage="csr": centring the columns makes D dense - scale the sparse matrix yourself'
    with pytest.raises(ValueError, match=old):
        rbl.ADMMmethod(A, y, "erm", "binary_cross_entropy", l1_reg=0.01, storage="csr", standardize=True)
    with pytest.raises(ValueError, match=old + r'.*standardize="scale"'):
        rbl.ADMMgroup(A, y, [dict(l2_reg=0.1, standardize=True)], storage="csr")


def test_nonzero_mean_with_csr_is_refused_before_any_device_call():
    _pkg()
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
    X, y = _data()
    A = sp.csr_matrix(X)
    mean = np.zeros(6)
    mean[4] = 1e-300
    with pytest.raises(ValueError, match=r'scaling with storage="csr": the mean vector must be all zeros'):
        calculate_accuracy(np.ones(6), A, y, scaling=(mean, np.ones(6)), storage="csr")
    with pytest.raises(ValueError, match=r'scaling with storage="csr": the mean vector must be all zeros'):
        calculate_accuracy(np.ones(7), A, y, scaling=(mean, np.ones(6)), storage="csr")       # (w carries an intercept)


# ------------------------------------------------------------------------------------------- the restated statistic
def test_degenerate_columns_get_scale_one():
    n = 2500                                             # a full column spans two segments
    for x in (np.full(n, 0.1), np.full(n, -3.7e8), np.array([]), np.zeros(7), -np.zeros(5), np.array([0.0, -0.0, 0.0])):
        st = ref.column_stat(x, n)
        assert st["var"] == 0.0 and st["scale"] == 1.0, x[:1]
    assert ref.column_stat(np.array([2.0]), n)["scale"] != 1.0          # (a single entry is not degenerate)


def test_exact_fixture_matches_numpy_in_bits():
    """small integers, n a power of two: every sum, the division by n and the squares are exact, so the scale is
    sqrt(var) of the exact variance - whatever the order of summation - and equals the dense restatement's"""
    n, d = 4096, 7
    rng = np.random.default_rng(5)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    M = rng.random((n, d)) < 0.4
    M[:, 0] = True                                       # a full varying column: two segments, shifted by its first row
    M[:, 1] = True
    X[:, 1] = 3.0                                        # a full constant column
    M[:, 2] = False                                      # an empty column
    X[:, 3] = 0.0                                        # explicit zeros only
    M[:, 4] = False
    M[17, 4] = True
    X[17, 4] = -2.0                                      # a single entry
    rows, cols = np.nonzero(M)
    A = sp.csr_matrix((X[rows, cols], cols, np.concatenate([[0], np.cumsum(M.sum(axis=1))])), shape=(n, d))
    assert A.nnz == M.sum() and (A.data == 0.0).sum() > n * 0.3
    mean, scale = ref.fit_csr(A)
    dense = A.toarray()
    want_mean, want_scale = scaling_ref.fit(dense)
    var = ((dense - dense.mean(axis=0)) ** 2).mean(axis=0)
    want = np.where(var > 0.0, np.sqrt(var), 1.0)
    assert np.array_equal(scale.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(scale.view(np.uint64), want_scale.view(np.uint64))
    assert np.array_equal(mean, want_mean)
    assert scale[1] == scale[2] == scale[3] == 1.0 and scale[0] != 1.0 and scale[4] != 1.0


def test_real_data_within_the_k_term_bound():
    """both sums of every column against np.longdouble sums of the same terms: |error| <= k 2^-53 sum |terms| (k terms, any
    order of summation; the reference's own error, about 2^-64 log2 k sum |terms|, is three orders below the bound).  The
    resulting scale against a longdouble two-pass variance of the same column."""
    n, d = 3000, 10
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-3, 4, size=d) + rng.standard_normal(d) * 5.0
    M = rng.random((n, d)) < np.linspace(0.02, 1.0, d)
    M[:, d - 1] = True                                   # a full column (shifted) of 3000 entries: two segments
    u = 2.0 ** -53
    for j in range(d):
        x = X[M[:, j], j]
        st = ref.column_stat(x, n)
        k = x.size
        assert st["cnt"] == k and (k == n) == (j == d - 1)
        for terms, got in ((st["terms1"], st["s1"]), (st["terms2"], st["s2"])):
            exact = np.sum(terms.astype(np.longdouble))
            bound = k * u * float(np.sum(np.abs(terms)))
            err = abs(float(np.longdouble(got) - exact))
            print(f"column {j}: k={k} error {err:.3e} bound {bound:.3e}")
            assert err <= bound
        # the scale: var is a sum of non-negative terms, so the errors above carry over relative to var - terms2 and
        # (n - cnt) m^2 are formed with a handful of roundings each (<= 8 u relative, m's own error included to first
        # order because the sum of (x - m) vanishes at the true mean), sqrt halves the relative error and adds u / 2
        col = np.zeros(n, dtype=np.longdouble)
        col[M[:, j]] = x
        var = np.mean((col - np.mean(col)) ** 2)
        rel = abs(float((np.longdouble(st["scale"]) - np.sqrt(var)) / np.sqrt(var)))
        bound = ((k + 8) * u) / 2 + u
        # a shifted full column: the terms are x - sh, conditioned like the spread, not like the values
        print(f"column {j}: scale {st['scale']:.17g} relative error {rel:.3e} bound {bound:.3e}")
        assert rel <= bound
