"""CPU-only checks of the typed data path (include/rbl.h: rbl_set_data_from, rbl_set_scaling, rbl_get_scaling):
_solver.as_source uses float64 / float32 / float16 arrays and torch CPU tensors in place, converts what the library has
no instance for, and refuses bfloat16; the three symbols are in header, library and binding with the ABI version
unchanged; the NumPy restatement of the scaling (tests/scaling_ref.py) agrees with sklearn.preprocessing.scale where
sklearn is installed and with a hand-computed case where it is not."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import scaling_ref


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.float16])
def test_as_source_uses_c_row_arrays_in_place(dt):
    rbl = _pkg()
    L = rbl._lib
    A = np.arange(35, dtype=dt).reshape(5, 7)
    s = rbl._solver.as_source(A)
    assert s.ptr == A.ctypes.data and s.keep is A                       # no copy
    assert (s.dtype, s.mem, s.ldx, s.shape) == (L.SOURCE_DTYPE[np.dtype(dt)], L.MEM_HOST, 7, (5, 7))
    # a column slice of a wider array: in place, with the wide array's row stride
    B = A[:, :4]
    s = rbl._solver.as_source(B)
    assert s.ptr == A.ctypes.data and (s.ldx, s.shape) == (7, (5, 4))
    C_ = A[1:, 2:5]
    s = rbl._solver.as_source(C_)
    assert s.ptr == C_.ctypes.data == A.ctypes.data + (7 + 2) * A.itemsize and (s.ldx, s.shape) == (7, (4, 3))
    # every second row: still whole rows at a positive stride
    s = rbl._solver.as_source(A[::2])
    assert s.ptr == A.ctypes.data and (s.ldx, s.shape) == (14, (3, 7))
    assert rbl._solver.as_source(s) is s


@pytest.mark.parametrize("dt", ["float64", "float32", "float16"])
def test_as_source_views_torch_cpu_tensors(dt):
    torch = pytest.importorskip("torch")
    rbl = _pkg()
    L = rbl._lib
    T = torch.arange(24, dtype=getattr(torch, dt)).reshape(4, 6)
    s = rbl._solver.as_source(T)
    assert s.ptr == T.data_ptr() and (s.dtype, s.mem, s.ldx, s.shape) == (L.SOURCE_DTYPE[np.dtype(dt)], L.MEM_HOST, 6, (4, 6))
    s = rbl._solver.as_source(T[:, 1:4])
    assert s.ptr == T[:, 1:4].data_ptr() and (s.ldx, s.shape) == (6, (4, 3))


def test_as_source_converts_what_has_no_instance():
    rbl = _pkg()
    L = rbl._lib
    A = np.arange(12, dtype=np.float32).reshape(3, 4)
    for X in (np.asfortranarray(A), A[::-1], A[:, ::2], A.astype(np.int32), A > 3, A.tolist(), A.astype(">f4")):
        s = rbl._solver.as_source(X)
        assert (s.dtype, s.mem, s.ldx, s.shape) == (L.DTYPE_F64, L.MEM_HOST, np.shape(X)[1], np.shape(X))
        assert isinstance(s.keep, np.ndarray) and s.keep.dtype == np.float64 and s.keep.flags["C_CONTIGUOUS"]
        assert s.ptr == s.keep.ctypes.data
        assert np.array_equal(s.keep, np.asarray(X, dtype=np.float64))
    with pytest.raises(ValueError, match="2-D"):
        rbl._solver.as_source(np.zeros(5))
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(np.zeros((2, 2), dtype=np.complex128))


def test_as_source_refuses_bfloat16_and_integer_tensors_convert():
    torch = pytest.importorskip("torch")
    rbl = _pkg()
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(torch.zeros(3, 2, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        rbl._solver.as_source(torch.zeros(3, 2, dtype=torch.complex64))
    s = rbl._solver.as_source(torch.arange(6, dtype=torch.int64).reshape(3, 2))
    assert s.dtype == rbl._lib.DTYPE_F64 and np.array_equal(s.keep, np.arange(6.0).reshape(3, 2))


def test_new_symbols_in_header_library_and_binding():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    lib = rbl._lib.load()
    for name in ("rbl_set_data_from", "rbl_set_scaling", "rbl_get_scaling"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in rbl._lib.SIGNATURES, name
    for name in ("RBL_DTYPE_F64 = 0, RBL_DTYPE_F32 = 1, RBL_DTYPE_F16 = 2", "RBL_MEM_HOST = 0, RBL_MEM_DEVICE = 1",
                 "RBL_SCALE_NONE = 0, RBL_SCALE_FIT = 1, RBL_SCALE_APPLY = 2", "RBL_DATA_ONES_COLUMN = 1"):
        assert name in header, name
    L = rbl._lib
    assert (L.DTYPE_F64, L.DTYPE_F32, L.DTYPE_F16, L.MEM_HOST, L.MEM_DEVICE, L.DATA_ONES_COLUMN) == (0, 1, 2, 0, 1, 1)
    assert L.SCALING == {"none": 0, "fit": 1, "apply": 2}
    assert "rbl_set_data" in L.SIGNATURES                               # the plain binding stays
    for m in ("set_data", "set_data_f64", "set_scaling", "get_scaling"):
        assert callable(getattr(rbl.Solver, m)), m
    assert lib.rbl_version() == 106
    assert "#define RBL_VERSION 106" in header


def test_python_surface_of_standardize():
    import inspect
    rbl = _pkg()
    for cls in (rbl.ADMMmethod, rbl.smoothADMMmethod, rbl.OneVsRest):
        p = inspect.signature(cls.__init__).parameters
        assert p["standardize"].default is False, cls
    assert "standardize" in rbl.ADMMgroup._KEYS
    assert callable(rbl.ADMMmethod.unscaled)
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
    from admm_for_rank_based_loss_amd.src.util.fair_metric import calculate_statistics
    assert inspect.signature(calculate_accuracy).parameters["scaling"].default is None
    assert inspect.signature(calculate_statistics).parameters["scaling"].default is None
    # members of one group share one data matrix: they all standardise or none does (checked before any device call)
    X, y = np.zeros((4, 2)), np.array([1.0, -1.0, 1.0, -1.0])
    with pytest.raises(ValueError, match="problem 1: standardize must be the same"):
        rbl.ADMMgroup(X, y, [dict(l2_reg=0.1, standardize=True), dict(l2_reg=0.2)])
    mean, scale = rbl._solver.as_scaling([1.0, 2.0], [3.0, 4.0], 3, ones_column=True)
    assert mean.tolist() == [1.0, 2.0, 0.0] and scale.tolist() == [3.0, 4.0, 1.0]
    with pytest.raises(ValueError, match="entries for 3 columns"):
        rbl._solver.as_scaling([1.0, 2.0], [3.0, 4.0], 3)


def test_scaling_ref_hand_case_and_sklearn():
    # 4 x 3 by hand: column 0 = (1, 2, 3, 4): mean 2.5, var (2.25 + 0.25 + 0.25 + 2.25) / 4 = 1.25; column 1 constant:
    # mean 7, zero variance -> scale 1; column 2 = (-2, 2, -2, 2): mean 0, var 4 -> scale 2
    X = np.array([[1.0, 7.0, -2.0], [2.0, 7.0, 2.0], [3.0, 7.0, -2.0], [4.0, 7.0, 2.0]])
    y = np.array([1.0, -1.0, -1.0, 1.0])
    mean, scale = scaling_ref.fit(X)
    assert mean.tolist() == [2.5, 7.0, 0.0]
    assert scale.tolist() == [np.sqrt(1.25), 1.0, 2.0]
    Z = scaling_ref.standardize(X, mean, scale)
    inv = 1.0 / np.sqrt(1.25)
    assert Z[:, 0].tolist() == [-1.5 * inv, -0.5 * inv, 0.5 * inv, 1.5 * inv]
    assert Z[:, 1].tolist() == [0.0] * 4 and Z[:, 2].tolist() == [-1.0, 1.0, -1.0, 1.0]
    D = scaling_ref.form_D(X, y, mean, scale, "f32", ones_column=True)
    assert D.shape == (4, 4) and D[:, 3].tolist() == [-1.0, 1.0, 1.0, -1.0]
    assert np.array_equal(D[:, :3], (-y[:, None] * Z).astype(np.float32).astype(np.float64))
    assert np.array_equal(scaling_ref.form_D(X, y, storage="fp16"), (-y[:, None] * X).astype(np.float16).astype(np.float64))
    try:
        from sklearn.preprocessing import scale as sk_scale
    except ImportError:
        return
    rng = np.random.default_rng(5)
    A = rng.standard_normal((300, 6)) * rng.uniform(0.1, 30.0, 6) + rng.uniform(-5.0, 5.0, 6)
    A[:, 2] = 4.0
    m, s = scaling_ref.fit(A)
    assert s[2] == 1.0
    assert np.allclose(scaling_ref.standardize(A, m, s), sk_scale(A), rtol=0, atol=1e-12)
