"""CPU-only checks of the group feature's host side: the new symbols exist in the header, the library and the
binding; ADMMgroup validates its arguments before any device call; without a GPU a valid group fails loudly."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ["rbl_create_shared", "rbl_group_create", "rbl_group_destroy", "rbl_group_step", "rbl_group_solve",
               "rbl_group_counters", "rbl_k_gemv_multi", "rbl_k_gemvt_multi"]


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def test_group_symbols_in_header_library_and_binding():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    declared = set(re.findall(r"\b(rbl_[A-Za-z0-9_]+)\s*\(", header))
    lib = rbl._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in rbl._lib.SIGNATURES, name
    assert "typedef struct rbl_group rbl_group;" in header
    assert lib.rbl_version() == 106          # the ABI version and the structure layouts are unchanged
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS[:6]:
        assert name in doc, name


def test_python_surface_exists():
    rbl = _pkg()
    assert callable(rbl.ADMMgroup) and "ADMMgroup" in rbl.__all__
    assert callable(rbl._solver.Group)
    for name in ("step", "solve", "counters"):
        assert callable(getattr(rbl._solver.Group, name))
    import inspect
    for cls in (rbl.ADMMmethod, rbl.smoothADMMmethod):
        params = list(inspect.signature(cls.__init__).parameters)
        assert params[-1] == "share_data", params            # one more TRAILING keyword
        assert inspect.signature(cls.__init__).parameters["share_data"].default is None
    assert "share" in inspect.signature(rbl._solver.Solver.__init__).parameters
    assert list(inspect.signature(rbl.ADMMgroup.__init__).parameters)[1:] == \
        ["X", "y", "problems", "storage", "device", "max_iter", "tol"]


def test_admmgroup_argument_validation_needs_no_device():
    rbl = _pkg()
    X = np.zeros((10, 2))
    y = np.ones((10, 1))
    ok = dict(weight_function="superquantile", l2_reg=0.1, args=[0.5])
    cases = [
        ([], "non-empty list"),
        (None, "non-empty list"),
        ([ok, dict(ok, lr=0.1)], r"problem 1: unknown keyword\(s\) \['lr'\]"),
        ([dict(weight_function="nope", l2_reg=0.1, args=[1])], "problem 0: Unrecognized framework 'nope'"),
        ([ok, dict(weight_function="superquantile", l2_reg=0.1)], "problem 1: args for framework is None!"),
        ([dict(weight_function="aorr_dc", l2_reg=0.1, args=[2, 5])], "problem 0: need args"),
        ([dict(loss="square", l2_reg=0.1)], "problem 0: Unrecognized loss 'square'"),
        ([dict(weight_function="ehrm", loss="hinge", l2_reg=0.1, B=-5)], "erhm only can be with the binary_cross_entropy."),
        ([dict(weight_function="erm", l2_reg=0.1, B=-5)], r"Unrecognized weight_function 'erm'! Options: \['ehrm'\]"),
        ([ok, ok, dict(weight_function="erm")], "problem 2: More arguments: l1_reg or l2_reg"),
        ([dict(ok, t=0.5)], "problem 0: t is the smoothing parameter"),
        ([ok] * 65, "at most 64"),
        (["superquantile"], "problem 0: expected a dict"),
    ]
    for problems, msg in cases:
        with pytest.raises(ValueError, match=msg):
            rbl.ADMMgroup(X, y, problems)
    with pytest.raises(ValueError, match="storage must be one of"):
        rbl.ADMMgroup(X, y, [ok], storage="f16")
    with pytest.raises(ValueError, match="at least one solver"):
        rbl._solver.Group([])


def test_group_has_no_cpu_fallback_without_device():
    rbl = _pkg()
    if rbl._lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.random.default_rng(0).standard_normal((20, 3))
    y = np.sign(X[:, :1])
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl.ADMMgroup(X, y, [dict(weight_function="erm", loss="hinge", l2_reg=0.1),
                             dict(weight_function="superquantile", l2_reg=0.1, args=[0.5])])
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl._lib.k_gemv_multi(np.ones((3, 2)), np.ones((2, 2)))
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl._lib.k_gemvt_multi(np.ones((3, 2)), np.ones((2, 3)))
