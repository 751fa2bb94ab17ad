"""CPU-only checks of the sparse data path (include/rbl.h: rbl_set_data_csr): _solver.as_source hands a canonical SciPy
CSR matrix / array and a torch sparse_csr tensor to the library in place (the caller's own three buffers), converts
other formats, non-canonical matrices, mixed index widths and integer data without touching the caller's object, and
refuses what the library has no instance for; the symbol is in header, library and binding; the host arithmetic of
the upload (csrc/csr_plan.h) passes its stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

sp = pytest.importorskip("scipy.sparse")


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def _random_csr(n, d, density, dtype, itype, seed=0, cls=None):
    rng = np.random.default_rng(seed)
    A = sp.random(n, d, density=density, format="csr", dtype=np.float64, random_state=rng).astype(dtype)
    A = (cls or sp.csr_matrix)(A)
    A.indices, A.indptr = A.indices.astype(itype), A.indptr.astype(itype)    # (the constructor narrows indices that fit int32)
    assert A.has_canonical_format and A.indices.dtype == A.indptr.dtype == np.dtype(itype)
    return A


@pytest.mark.parametrize("cls", ["csr_matrix", "csr_array"])
@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_canonical_scipy_csr_is_used_in_place(dt, itype, cls):
    rbl = _pkg()
    L = rbl._lib
    A = _random_csr(13, 7, 0.3, dt, itype, cls=getattr(sp, cls))
    s = rbl._solver.as_source(A)
    assert isinstance(s, rbl._solver.CsrSource)
    assert (s.indptr, s.indices, s.values) == (A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data)   # no copy
    assert s.shape == (13, 7) and s.nnz == A.nnz and s.mem == L.MEM_HOST
    assert s.dtype == L.SOURCE_DTYPE[np.dtype(dt)] and s.index_type == L.INDEX_DTYPE[np.dtype(itype)]
    assert rbl._solver.as_source(s) is s
    # the dense Source is what it was
    d = rbl._solver.as_source(A.toarray())
    assert isinstance(d, rbl._solver.Source) and d.ldx == 7


def _snapshot(A):
    if A.format == "coo":
        return [A.row.copy(), A.col.copy(), A.data.copy()]
    return [A.indptr.copy(), A.indices.copy(), A.data.copy()]


def _csr_of(s):
    """the CSR matrix a host CsrSource describes, rebuilt from its three addresses"""
    import ctypes as C
    rbl = _pkg()
    it = np.int64 if s.index_type == rbl._lib.INDEX_I64 else np.int32
    vt = {v: k for k, v in rbl._lib.SOURCE_DTYPE.items()}[s.dtype]

    def arr(addr, count, dt):
        if count == 0:
            return np.zeros(0, dtype=dt)
        return np.frombuffer((C.c_char * (count * np.dtype(dt).itemsize)).from_address(addr), dtype=dt).copy()
    return sp.csr_matrix((arr(s.values, s.nnz, vt), arr(s.indices, s.nnz, it), arr(s.indptr, s.shape[0] + 1, it)), shape=s.shape)


def test_other_formats_and_non_canonical_input_are_converted_and_left_untouched():
    rbl = _pkg()
    L = rbl._lib
    A = _random_csr(11, 9, 0.4, np.float64, np.int32, seed=3)
    dense = A.toarray()
    # non-canonical: row 2's indices reversed, and a duplicate pair in row 5 (same column twice)
    indptr, indices, data = A.indptr.copy(), A.indices.copy(), A.data.copy()
    a, b = indptr[2], indptr[3]
    assert b - a >= 2
    indices[a:b], data[a:b] = indices[a:b][::-1].copy(), data[a:b][::-1].copy()
    unsorted = sp.csr_matrix((data, indices, indptr), shape=A.shape)
    row = np.array([0, 5, 5, 5, 10]); col = np.array([1, 4, 4, 2, 8]); val = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    dup = sp.csr_matrix((val, col, np.array([0, 1, 1, 1, 1, 1, 4, 4, 4, 4, 4, 5])), shape=(11, 9))
    coo = sp.coo_matrix((val, (row, col)), shape=(11, 9))
    dup_dense = np.zeros((11, 9)); np.add.at(dup_dense, (row, col), val)
    cases = [(A.tocsc(), dense), (A.tocoo(), dense), (unsorted, dense), (dup, dup_dense), (coo, dup_dense),
             (A.tolil(), dense)]
    for M, want in cases:
        before = _snapshot(M) if M.format in ("csr", "csc", "coo") else None
        s = rbl._solver.as_source(M)
        assert isinstance(s, rbl._solver.CsrSource) and s.mem == L.MEM_HOST and s.shape == (11, 9), M.format
        got = _csr_of(s)
        assert got.has_canonical_format, M.format
        assert np.array_equal(got.toarray(), want), M.format
        if before is not None:                           # the caller's object: the same arrays, the same contents
            assert all(np.array_equal(x, y) for x, y in zip(before, _snapshot(M))), M.format
    assert np.array_equal(unsorted.indices, indices) and np.array_equal(dup.indices, col)


def test_mixed_index_widths_become_int64_and_integer_data_float64():
    rbl = _pkg()
    L = rbl._lib
    A = _random_csr(6, 5, 0.5, np.float32, np.int32, seed=5)
    M = sp.csr_matrix(A.shape, dtype=np.float32)
    M.data, M.indices, M.indptr = A.data, A.indices.astype(np.int32), A.indptr.astype(np.int64)   # set past the constructor
    if M.indices.dtype != M.indptr.dtype:                # (SciPy keeps what it is handed here)
        s = rbl._solver.as_source(M)
        assert s.index_type == L.INDEX_I64 and s.dtype == L.DTYPE_F32
        assert s.values == A.data.ctypes.data            # the values still in place
        assert np.array_equal(_csr_of(s).toarray(), A.toarray())
    for dt in (np.int64, np.int8, np.uint16, bool):
        I = sp.csr_matrix((np.arange(1, 4).astype(dt), np.array([0, 2, 1]), np.array([0, 2, 2, 3])), shape=(3, 3))
        s = rbl._solver.as_source(I)
        assert s.dtype == L.DTYPE_F64 and s.nnz == 3
        assert np.array_equal(_csr_of(s).toarray(), I.toarray().astype(np.float64))
    E = sp.csr_matrix((4, 3), dtype=np.float32)          # nnz == 0
    s = rbl._solver.as_source(E)
    assert s.nnz == 0 and s.shape == (4, 3) and s.dtype == L.DTYPE_F32
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(sp.csr_matrix((2, 2), dtype=np.complex128))


@pytest.mark.parametrize("dt", ["float64", "float32", "float16"])
@pytest.mark.parametrize("itype", ["int32", "int64"])
def test_torch_cpu_sparse_csr_is_used_in_place(dt, itype):
    import torch
    rbl = _pkg()
    L = rbl._lib
    crow = torch.tensor([0, 2, 2, 5], dtype=getattr(torch, itype))
    col = torch.tensor([0, 3, 1, 2, 3], dtype=getattr(torch, itype))
    val = torch.tensor([1.0, -2.0, 0.5, 4.0, -0.0], dtype=getattr(torch, dt))
    T = torch.sparse_csr_tensor(crow, col, val, size=(3, 4))
    s = rbl._solver.as_source(T)
    assert isinstance(s, rbl._solver.CsrSource)
    assert (s.indptr, s.indices, s.values) == (T.crow_indices().data_ptr(), T.col_indices().data_ptr(), T.values().data_ptr())
    assert s.shape == (3, 4) and s.nnz == 5 and s.mem == L.MEM_HOST
    assert s.dtype == L.SOURCE_DTYPE[np.dtype(dt)] and s.index_type == L.INDEX_DTYPE[np.dtype(itype)]


def test_torch_coo_and_csc_are_converted_and_unsupported_tensors_refused():
    import torch
    rbl = _pkg()
    dense = torch.tensor([[0.0, 1.5, 0.0], [2.0, 0.0, -3.0]], dtype=torch.float32)
    for T in (dense.to_sparse(), dense.to_sparse_csc()):
        s = rbl._solver.as_source(T)
        assert isinstance(s, rbl._solver.CsrSource) and s.nnz == 3 and s.dtype == rbl._lib.DTYPE_F32
        assert np.array_equal(_csr_of(s).toarray(), dense.numpy())
    coo = torch.sparse_coo_tensor(torch.tensor([[0, 0, 1], [1, 1, 2]]), torch.tensor([1.0, 2.0, 3.0]), size=(2, 3))   # a duplicate
    assert np.array_equal(_csr_of(rbl._solver.as_source(coo)).toarray(), np.array([[0, 3.0, 0], [0, 0, 3.0]]))
    crow, col = torch.tensor([0, 1, 2]), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(torch.sparse_csr_tensor(crow, col, torch.ones(2, dtype=torch.bfloat16), size=(2, 2)))
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(torch.sparse_csr_tensor(crow, col, torch.ones(2, dtype=torch.complex64), size=(2, 2)))
    batched = torch.sparse_csr_tensor(torch.stack([crow, crow]), torch.stack([col, col]), torch.ones(2, 2), size=(2, 2, 2))
    with pytest.raises(ValueError, match="2-D"):
        rbl._solver.as_source(batched)


def test_baselines_densify_sparse_input():
    rbl = _pkg()
    A = _random_csr(5, 4, 0.5, np.float32, np.int32, seed=7)
    M = rbl._solver._as_matrix(A)
    assert M.dtype == np.float64 and M.flags["C_CONTIGUOUS"] and np.array_equal(M, A.toarray())


def test_symbol_is_declared_exported_and_bound():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    assert "rbl_set_data_csr(" in header and "RBL_INDEX_I32 = 0, RBL_INDEX_I64 = 1" in header
    assert "#define RBL_VERSION 106" in header           # the symbol is the capability probe
    assert "rbl_set_data_csr" in rbl._lib.SIGNATURES and len(rbl._lib.SIGNATURES["rbl_set_data_csr"][1]) == 11
    assert hasattr(rbl._lib.load(), "rbl_set_data_csr")
    assert (rbl._lib.INDEX_I32, rbl._lib.INDEX_I64) == (0, 1)


def test_csr_plan_program_passes_under_the_sanitizers(tmp_path):
    """chunk boundaries, the fullest chunk, the rebasing offsets (int32 and int64 indptr, empty rows and chunks) and the
    structure checks on indptr: the stand-alone program replays every chunk in buffers of the planned sizes"""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "csr_plan_main")
    src = os.path.join(ROOT, "tests", "csr_plan_main.cpp")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and ("cannot find" in cc.stderr or "unsupported" in cc.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "csr_plan: ok" in run.stdout, run.stdout + run.stderr
