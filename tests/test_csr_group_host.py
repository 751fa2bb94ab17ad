"""Groups with shared sparse passes (storage="csr", RBL_GROUP_SHARE_SPARSE), the part that needs no GPU: the new symbols
in header, library and binding, the argument check of ``share_sparse`` and the flag check of rbl_group_create_opts, both
of which come before any device call.  ADMMgroup's constructor signature is pinned (tests/test_group_host.py), so the
group-wide option travels in the problem dicts, as ``standardize`` and ``fit_intercept`` do; OneVsRest and
_solver.Group take it as a keyword."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def test_symbols_are_declared_exported_and_bound():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    declared = set(re.findall(r"\b(rbl_[A-Za-z0-9_]+)\s*\(", header))
    lib = rbl._lib.load()
    for name in ("rbl_group_create_opts", "rbl_k_csr_gemv_multi", "rbl_k_csr_gemvt_multi", "rbl_group_profile", "rbl_group_pass_times"):
        assert name in declared and name in rbl._lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+RBL_GROUP_SHARE_SPARSE\s+1\b", header) and rbl._lib.GROUP_SHARE_SPARSE == 1
    assert len(rbl._lib.SIGNATURES["rbl_group_create_opts"][1]) == len(rbl._lib.SIGNATURES["rbl_group_create"][1]) + 1
    assert len(rbl._lib.SIGNATURES["rbl_k_csr_gemv_multi"][1]) == len(rbl._lib.SIGNATURES["rbl_k_csr_gemvt_multi"][1]) == 10
    assert callable(rbl._lib.k_csr_gemv_multi) and callable(rbl._lib.k_csr_gemvt_multi)
    assert callable(rbl._solver.Group.profile) and callable(rbl._solver.Group.pass_times)


@pytest.mark.parametrize("value", [1, 0, "yes", None, 1.0, [True]])
def test_share_sparse_must_be_a_bool(value, monkeypatch):
    rbl = _pkg()

    def no_device(*a, **k):
        raise AssertionError("a device call before the argument check")

    monkeypatch.setattr(rbl._lib, "load", no_device)        # every call into the library goes through it
    X, y = np.zeros((6, 3)), np.array([1.0, -1.0] * 3)
    with pytest.raises(ValueError, match="share_sparse must be True or False"):
        rbl.ADMMgroup(X, y, [dict(l2_reg=0.1), dict(l2_reg=0.2, share_sparse=value)])
    with pytest.raises(ValueError, match="share_sparse must be True or False"):
        rbl.OneVsRest(X, np.arange(6) % 3, l2_reg=0.1, share_sparse=value)
    with pytest.raises(ValueError, match="share_sparse must be True or False"):
        rbl._solver.Group([], share_sparse=value)


def test_share_sparse_is_one_option_for_the_whole_group(monkeypatch):
    rbl = _pkg()
    monkeypatch.setattr(rbl._lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    X, y = np.zeros((6, 3)), np.array([1.0, -1.0] * 3)
    assert "share_sparse" in rbl.ADMMgroup._KEYS
    with pytest.raises(ValueError, match="problem 1: share_sparse must be the same for every problem"):
        rbl.ADMMgroup(X, y, [dict(l2_reg=0.1, share_sparse=True), dict(l2_reg=0.2)])
    import inspect
    assert inspect.signature(rbl.OneVsRest.__init__).parameters["share_sparse"].default is False
    assert inspect.signature(rbl._solver.Group.__init__).parameters["share_sparse"].default is False


def test_unknown_flag_bits_are_refused_before_anything_else():
    """no members, no device: the flag check comes first, and *out is cleared"""
    L = _pkg()._lib
    lib = L.load()
    for flags in (2, 3, 4, 1 << 30, -2):
        out = C.c_void_p(12345)
        assert lib.rbl_group_create_opts(None, 0, flags, C.byref(out)) == L.RBL_ERR_INVALID
        assert "unknown flag bits" in L.last_error() and out.value is None
    out = C.c_void_p(12345)
    for flags in (0, 1):            # a known flag gets as far as the member check
        assert lib.rbl_group_create_opts(None, 0, flags, C.byref(out)) == L.RBL_ERR_INVALID
        assert "1..64 members" in L.last_error()
    assert lib.rbl_group_create(None, 0, C.byref(out)) == L.RBL_ERR_INVALID and "1..64 members" in L.last_error()
