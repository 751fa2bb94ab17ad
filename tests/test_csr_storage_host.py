"""Sparse storage (storage="csr", RBL_STORE_CSR), the part that needs no GPU: the storage table against the C header, the
row-stride and rounding helpers, the Python refusals (a dense X or X_test, standardize=True) before any device call, the
new symbols in header, library and binding, and the segment plan of q = D^T c (csrc/csc_plan.h) replayed by a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

sp = pytest.importorskip("scipy.sparse")


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def test_storage_table_matches_the_header():
    L = _pkg()._lib
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    assert re.findall(r"RBL_STORE_CSR = (\d+)", text) == ["3"]
    assert L.STORAGE["csr"] == L.STORE_CSR == 3
    assert sorted(set(L.STORAGE.values())) == [0, 1, 2, 3]
    assert [k for k, v in L.STORAGE.items() if v == 3] == ["csr"]          # the single new key
    assert "#define RBL_VERSION 106" in text


def test_storage_ld_and_round():
    L = _pkg()._lib
    for d in (1, 3, 4, 5, 39, 40, 1000, 1001, 4100, 16384):
        assert L.storage_ld(d, "csr") == L.storage_ld(d, "f64")
    rng = np.random.default_rng(0)
    X = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-300, 300, 500), [0.0, -0.0, 1e-320, 7e4, np.inf]])
    R = L.storage_round(X.reshape(-1, 1), "csr")
    assert R.dtype == np.float64 and np.array_equal(R.view(np.uint64).reshape(-1), X.view(np.uint64))   # the identity


def test_symbols_are_declared_exported_and_bound():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    declared = set(re.findall(r"\b(rbl_[A-Za-z0-9_]+)\s*\(", header))
    lib = rbl._lib.load()
    for name in ("rbl_k_csr_gemv", "rbl_k_csr_gemvt", "rbl_k_csr_gram"):
        assert name in declared and name in rbl._lib.SIGNATURES and hasattr(lib, name), name
        assert callable(getattr(rbl._lib, name[4:]))
    assert lib.rbl_version() == 106


def _data(n=30, d=6):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.3)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return X, y


def test_dense_X_is_refused_before_any_device_call():
    rbl = _pkg()
    X, y = _data()
    msg = r'storage="csr" needs a sparse X .* scipy\.sparse\.csr_matrix\(X\)'
    with pytest.raises(ValueError, match=msg):
        rbl.ADMMmethod(X, y, "erm", "binary_cross_entropy", l1_reg=0.01, storage="csr")
    with pytest.raises(ValueError, match=msg):
        rbl.smoothADMMmethod(X.astype(np.float32), y, "erm", "hinge", l1_reg=0.01, storage="csr")
    with pytest.raises(ValueError, match=msg):
        rbl.ADMMgroup(X, y, [dict(weight_function="superquantile", l2_reg=0.1, args=[0.5])], storage="csr")
    with pytest.raises(ValueError, match=msg):
        rbl.OneVsRest(X, np.arange(X.shape[0]) % 3, l2_reg=0.1, storage="csr")
    import torch
    with pytest.raises(ValueError, match=msg):
        rbl.ADMMmethod(torch.from_numpy(X), y, "erm", "binary_cross_entropy", l1_reg=0.01, storage="csr")


def test_dense_X_test_is_refused_before_any_device_call():
    rbl = _pkg()
    X, y = _data()
    with pytest.raises(ValueError, match=r'storage="csr" needs a sparse X_test .* scipy\.sparse\.csr_matrix\(X_test\)'):
        rbl.rankbasedObjective(X, y, "erm", "binary_cross_entropy", storage="csr")      # what start_store builds
    # start_store itself, on an object that never reached a device
    s = object.__new__(rbl.ADMMmethod)
    s._storage, s._device, s._scaling, s.fit_intercept, s._pen = "csr", 0, None, False, None
    with pytest.raises(ValueError, match=r"scipy\.sparse\.csr_matrix\(X_test\)"):
        s.start_store(X, y)
    o = object.__new__(rbl.OneVsRest)
    o._storage, o._device, o.fit_intercept, o.W, o._test = "csr", 0, False, np.zeros((X.shape[1], 3)), None
    with pytest.raises(ValueError, match=r"scipy\.sparse\.csr_matrix\(X_test\)"):
        o.predict(X)


def test_standardize_is_refused_before_any_device_call():
    rbl = _pkg()
    X, y = _data()
    A = sp.csr_matrix(X)
    with pytest.raises(ValueError, match=r'standardize=True with storage="csr": centring the columns makes D dense'):
        rbl.ADMMmethod(A, y, "erm", "binary_cross_entropy", l1_reg=0.01, storage="csr", standardize=True)
    with pytest.raises(ValueError, match=r'standardize=True with storage="csr"'):
        rbl.OneVsRest(A, np.arange(X.shape[0]) % 3, l2_reg=0.1, storage="csr", standardize=True)
    with pytest.raises(ValueError, match=r'standardize=True with storage="csr"'):
        rbl.rankbasedObjective(A, y, "erm", "binary_cross_entropy", storage="csr", scaling=(np.zeros(6), np.ones(6)))


def test_sparse_X_reaches_the_library():
    """a sparse X with storage="csr" passes every host check: without a GPU the first device call says so"""
    rbl = _pkg()
    if rbl._lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X, y = _data()
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl.ADMMmethod(sp.csr_matrix(X), y, "erm", "binary_cross_entropy", l1_reg=0.01, storage="csr", fit_intercept=True)


def test_csc_plan_program_passes_under_the_sanitizers(tmp_path):
    """every entry in exactly one segment, no segment across a column or longer than T, a column's segments consecutive
    and in order - for column lengths 0, 1, T - 1, T, T + 1, 2T + 1 and one column holding every entry, T = 64 .. 2048"""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "csc_plan_main")
    src = os.path.join(ROOT, "tests", "csc_plan_main.cpp")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and ("cannot find" in cc.stderr or "unsupported" in cc.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "csc_plan: ok" in run.stdout, run.stdout + run.stderr
