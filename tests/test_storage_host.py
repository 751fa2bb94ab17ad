"""fp16 storage, the part that needs no GPU: the storage table against the C header, the row stride rule, the rounding
helper (``_lib.storage_round`` forms "the matrix the device stores"), and what rounding the data costs - measured with the
CPU oracle alone, which is the figure DESIGN.md quotes."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    import admm_for_rank_based_loss_amd as rbl
    return rbl._lib


def test_storage_table_matches_the_header(L):
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(RBL_STORE_F\d+) = (\d+)", text))
    assert enum == {"RBL_STORE_F32": 0, "RBL_STORE_F64": 1, "RBL_STORE_F16": 2}
    assert L.STORAGE["fp16"] == L.STORAGE["float16"] == enum["RBL_STORE_F16"]
    assert L.STORAGE["f32"] == L.STORAGE["float32"] == 0 and L.STORAGE["f64"] == L.STORAGE["float64"] == 1
    assert "f16" not in L.STORAGE          # tests/test_group_host.py's example of a rejected name


def test_storage_ld(L):
    # whole 16-byte packets: 4 elements with f32 (and f64, which keeps the same stride), 8 with fp16
    for d, ld4, ld8 in [(1, 4, 8), (3, 4, 8), (4, 4, 8), (5, 8, 8), (7, 8, 8), (8, 8, 8), (9, 12, 16), (12, 12, 16),
                        (13, 16, 16), (16, 16, 16), (17, 20, 24), (333, 336, 336), (1000, 1000, 1000), (1001, 1004, 1008),
                        (1004, 1004, 1008), (1005, 1008, 1008)]:
        assert L.storage_ld(d, "f32") == ld4 and L.storage_ld(d, "f64") == ld4, d
        assert L.storage_ld(d, "fp16") == L.storage_ld(d, "float16") == ld8, d
    with pytest.raises(KeyError):
        L.storage_ld(8, "f16")


def test_storage_round(L):
    rng = np.random.default_rng(0)
    X = np.concatenate([rng.standard_normal(5000) * 10.0 ** rng.integers(-9, 5, 5000),
                        [0.0, -0.0, 65504.0, -65504.0, 65519.99, 1e-8, -1e-8, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                         6.1e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]]).reshape(-1, 1)
    X = X[np.abs(X[:, 0]) < 65520.0]
    R = L.storage_round(X, "fp16")
    assert R.dtype == np.float64 and R.shape == X.shape
    assert np.array_equal(R.view(np.uint64), X.astype(np.float16).astype(np.float64).view(np.uint64))   # bit-equal
    assert np.array_equal(L.storage_round(R, "fp16"), R)                                                # idempotent
    assert np.array_equal(L.storage_round(X, "f32"), X.astype(np.float32).astype(np.float64))
    assert L.storage_round(X, "f64") is not None and np.array_equal(L.storage_round(X, "f64"), X)
    assert L.storage_round(np.array([65504.0]), "fp16")[0] == 65504.0
    assert L.storage_round(np.array([1e-8]), "fp16")[0] == 0.0                  # underflow is rounding, not an error
    with pytest.raises(ValueError, match=r"fp16 storage: 2 finite entries do not fit float16 .* first at index \(0, 1\)"):
        L.storage_round(np.array([[1.0, 7e4, 3.0], [-1e5, 0.0, 0.0]]), "fp16")
    assert np.isinf(L.storage_round(np.array([np.inf, 1.0]), "fp16")[0])        # an infinite input is not "made" infinite


def _solve(L, X, y, storage, kw, **extra):
    from oracle import admm
    return admm.admm_solve(L.storage_round(X, storage), y, mode="exact", **extra, **kw)


def test_cost_of_rounding_the_data_erm(L):
    """erm / BCE / l1 on 600 x 40: the relative change of the final objective when the data are rounded to f32 and to
    fp16.  Recorded: all three solves stop after 127 iterations at F = 0.56608788; f32 8.9e-11, fp16 5.9e-7."""
    from oracle import problems
    X, y = problems.make_problem(600, 40, seed=3)
    kw = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01)
    F = {s: _solve(L, X, y, s, kw, tol=1e-6).final_objective for s in ("f64", "f32", "fp16")}
    d32, d16 = abs(F["f32"] - F["f64"]) / abs(F["f64"]), abs(F["fp16"] - F["f64"]) / abs(F["f64"])
    print(f"erm/BCE/l1 600x40: F = {F['f64']:.8f}, max|X| = {np.max(np.abs(X)):.2f}; relative difference f32 {d32:.2e}, fp16 {d16:.2e}")
    assert np.isfinite(d32) and np.isfinite(d16)
    assert d16 > d32


def test_cost_of_rounding_the_data_superquantile(L):
    """superquantile 0.5 / BCE / l2 0.01 on 600 x 40, 100 iterations with tol = 0 (no stop rule is met inside a few hundred
    iterations on problems of this kind, so the count is fixed; w is away from 0: max |w| = 3.4e-3).  Recorded:
    F = 0.69413552; f32 2.5e-11, fp16 2.3e-7.  fp16 perturbs an entry 2^13 times as much as f32 does."""
    from oracle import problems
    X, y = problems.make_problem(600, 40, seed=3)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    R = {s: _solve(L, X, y, s, kw, tol=0.0, max_iter=100) for s in ("f64", "f32", "fp16")}
    F = {s: r.final_objective for s, r in R.items()}
    assert all(len(r.primal) == 100 for r in R.values()) and np.max(np.abs(R["f64"].w)) > 1e-3
    d32, d16 = abs(F["f32"] - F["f64"]) / abs(F["f64"]), abs(F["fp16"] - F["f64"]) / abs(F["f64"])
    print(f"superquantile/BCE/l2 600x40, 100 iterations: F = {F['f64']:.8f}; relative difference f32 {d32:.2e}, fp16 {d16:.2e}")
    assert np.isfinite(d32) and np.isfinite(d16)
    assert d16 > d32
