"""The operator w-step (gram="none": a handle created with RBL_CREATE_NO_GRAM) without a GPU: the NumPy / SciPy restatement
(tests/wstep_op_ref.py) against dense solves and the lasso KKT conditions, the public header, the Python refusals - raised
before any device call - and the chunk plan of the d-space kernels replayed under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import wstep_op_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rbl.h")).read()


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def _small():
    A = ref.small_matrix()
    rng = np.random.default_rng(3)
    q = A.T @ rng.standard_normal(A.shape[0])
    return A, q, rng


def test_small_matrix_has_its_special_rows_and_columns():
    A = ref.small_matrix()
    assert A.shape == (300, 37)
    assert A[5].nnz == 0 and A[:, 11].nnz == 0
    col = A[:, 36].toarray().reshape(-1)
    assert np.all(np.delete(col, 5) == 1.0)
    assert 0.15 < A.nnz / (300 * 37) < 0.3


def test_restated_cg_against_a_dense_solve():
    A, q, rng = _small()
    d = A.shape[1]
    G = (A.T @ A).toarray()
    rho = 0.37
    l2 = rng.uniform(0.1, 2.0, d)
    l2[36] = 0.0                                  # the column of ones is free
    for reg, l2v in ((0.5, None), (0.0, l2)):
        w, it, ok = ref.cg(A, q, rho, reg, l2v, tol=1e-13)
        assert ok and it > 0
        dense = np.linalg.solve(rho * G + (reg * np.eye(d) if l2v is None else np.diag(l2v)), rho * q)
        assert np.max(np.abs(w - dense)) <= 1e-10 * max(1.0, np.max(np.abs(dense)))
        assert ref.ridge_residual(A, q, rho, reg, l2v, w) <= 1e-9


def test_wide_exact_ridge_is_the_dense_solve():
    """the n x n identity with a Schur complement for the free coordinate, on a shape where the dense solve is cheap"""
    D = ref.wide_matrix(60, 203, per_row=5, seed=4, ones_column=True)
    rng = np.random.default_rng(5)
    q = D.T @ rng.standard_normal(60)
    rho = 2.5e-3
    b = rng.uniform(0.05, 1.0, 203)
    for free in (False, True):
        bb = b.copy()
        if free:
            bb[202] = 0.0
        w = ref.ridge_exact_wide(D, q, rho, bb)
        dense = np.linalg.solve(rho * (D.T @ D).toarray() + np.diag(bb), rho * q)
        assert np.max(np.abs(w - dense)) <= 1e-11 * max(1.0, np.max(np.abs(dense)))


def test_restated_fista_meets_the_lasso_kkt_conditions():
    A, q, rng = _small()
    d = A.shape[1]
    rho = 0.37
    qm = float(np.max(np.abs(q)))
    bar = 1e-9 * max(1.0, qm)
    w, it, ok = ref.fista(A, q, rho, reg=2 * rho * 0.2 * qm, tol=1e-13)
    assert ok and 0 < np.count_nonzero(w) < d
    assert ref.enet_kkt(A, q, rho, 2 * rho * 0.2 * qm, None, w) <= bar
    l1 = 2 * rho * 0.2 * qm * rng.uniform(0.5, 2.0, d)
    l1[36] = 0.0
    l2 = rho * rng.uniform(0.0, 1.0, d)
    w, it, ok = ref.fista(A, q, rho, l1=l1, l2=l2, tol=1e-13)
    assert ok and w[36] != 0.0
    assert ref.enet_kkt(A, q, rho, l1, l2, w) <= bar


def test_restated_power_iteration_bounds_the_spectrum():
    A = ref.small_matrix()
    lam = float(np.linalg.eigvalsh((A.T @ A).toarray())[-1])
    L = ref.power_L(A)
    assert lam <= L <= 1.03 * lam


def test_header_declares_the_new_symbols_and_keeps_its_version():
    assert re.search(r"#define\s+RBL_VERSION\s+106\b", HEADER)
    assert re.search(r"#define\s+RBL_CREATE_NO_GRAM\s+1\b", HEADER)
    assert re.search(r"int\s+rbl_create_opts\(const rbl_config\* cfg, uint32_t flags, rbl_solver\*\* out\);", HEADER)
    assert re.search(r"int\s+rbl_k_wstep_op\(int wstep, int64_t n, int64_t d, const int64_t\* indptr", HEADER)
    assert "4 = the operator route" in HEADER


SIZES = (136, 112, 80, 56)   # rbl_config, rbl_stats, rbl_wstep_report, rbl_gram_report: as before this route existed


def test_struct_sizes_are_unchanged():
    """the layouts the header documents: rbl_config, rbl_stats and the two reports as the binding mirrors them"""
    import ctypes as C
    lib = _pkg()._lib
    assert (C.sizeof(lib.RblConfig), C.sizeof(lib.RblStats), C.sizeof(lib.RblWstepReport), C.sizeof(lib.RblGramReport)) == SIZES
    if os.path.exists(lib.LIB_PATH):
        so = C.CDLL(lib.LIB_PATH)
        assert tuple(so.rbl_sizeof(k) for k in range(4)) == SIZES
        assert so.rbl_version() == 106
        assert hasattr(so, "rbl_create_opts") and hasattr(so, "rbl_k_wstep_op")


def _xy(d=12, n=30):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, d))
    X[np.abs(X) < 0.8] = 0.0
    return X, np.where(rng.standard_normal(n) > 0, 1.0, -1.0)


def test_resolve_gram_rule():
    s = _pkg()._solver
    assert s.resolve_gram("auto", "f32", 50000) == "dense"
    assert s.resolve_gram("auto", "csr", 16384) == "dense"
    assert s.resolve_gram("auto", "csr", 16385) == "none"         # ld = 16388
    assert s.resolve_gram("auto", "csr", 16381) == "dense"        # ld = 16384
    assert s.resolve_gram("none", "csr", 10) == "none"
    assert s.resolve_gram("dense", "csr", 16384) == "dense"
    with pytest.raises(ValueError, match=r'gram="none" needs storage="csr"'):
        s.resolve_gram("none", "f64", 10)
    with pytest.raises(ValueError, match=r'gram="dense" with storage="csr" and 16385'):
        s.resolve_gram("dense", "csr", 16385)
    with pytest.raises(ValueError, match="gram must be one of"):
        s.resolve_gram("sparse", "csr", 10)


def test_python_refusals_come_before_any_device_call(monkeypatch):
    rbl = _pkg()

    def boom():
        raise AssertionError("the library was loaded: a device call was about to be made")

    monkeypatch.setattr(rbl._lib, "load", boom)
    X, y = _xy()
    A = sp.csr_matrix(X)
    with pytest.raises(ValueError, match=r'gram="none" needs storage="csr"'):
        rbl.ADMMmethod(X, y, "erm", "binary_cross_entropy", l2_reg=0.1, storage="f32", gram="none")
    with pytest.raises(ValueError, match="gram must be one of"):
        rbl.ADMMmethod(A, y, "erm", "binary_cross_entropy", l2_reg=0.1, storage="csr", gram="sparse")
    wide = sp.csr_matrix((np.ones(3), (np.arange(3), np.array([0, 5, 16384]))), shape=(3, 16385))
    with pytest.raises(ValueError, match=r'gram="dense" with storage="csr" and 16385'):
        rbl.ADMMmethod(wide, np.array([1.0, -1.0, 1.0]), "erm", "binary_cross_entropy", l2_reg=0.1, storage="csr", gram="dense")
    with pytest.raises(ValueError, match=r'gram must be "auto" or "dense"'):
        rbl.smoothADMMmethod(A, y, "erm", "binary_cross_entropy", l1_reg=0.1, storage="csr", gram="none")
    with pytest.raises(ValueError, match="smoothADMMmethod needs the Gram matrix"):
        rbl.smoothADMMmethod(wide, np.array([1.0, -1.0, 1.0]), "erm", "binary_cross_entropy", l1_reg=0.1, storage="csr")
    with pytest.raises(ValueError, match=r'gram="none" needs storage="csr"'):
        rbl.OneVsRest(X, np.arange(X.shape[0]) % 3, l2_reg=0.1, storage="f64", gram="none")
    with pytest.raises(ValueError, match="problem 1: gram must be the same for every problem"):
        rbl.ADMMgroup(A, y, [dict(l2_reg=0.1, gram="none"), dict(l2_reg=0.2, gram="dense")], storage="csr")
    with pytest.raises(ValueError, match="problem 0: gram must be one of"):
        rbl.ADMMgroup(A, y, [dict(l2_reg=0.1, gram=1)], storage="csr")
    with pytest.raises(ValueError, match=r'problem 0: smooth=True members have no gram="none" route'):
        rbl.ADMMgroup(A, y, [dict(l1_reg=0.1, smooth=True, gram="none")], storage="csr")
    with pytest.raises(ValueError, match=r'problem 0: gram="none" needs storage="csr"'):
        rbl.ADMMgroup(X, y, [dict(l2_reg=0.1, gram="none")], storage="f32")


def test_chunk_plan_program_passes_under_the_sanitizers(tmp_path):
    """every element of a vector in exactly one packet of one chunk, none beyond ld, one partial per chunk for any grid -
    at ld = 4, 40, C - 4, C, C + 4, 2C + 4, the first widths past the Gram route's cap, 10^6; the sum's order replayed"""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wstep_op_plan_main")
    src = os.path.join(ROOT, "tests", "wstep_op_plan_main.cpp")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and ("cannot find" in cc.stderr or "unsupported" in cc.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "wstep_op_plan: ok" in run.stdout, run.stdout + run.stderr
