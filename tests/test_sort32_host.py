"""What the GPU tests of the 32-bit-key sort (test_gpu_sort32.py) claim about their inputs, pinned on a CPU with the
NumPy restatement of the key map (oracle/sort32.py): the longest run of equal keys of every fixture, which fixtures must
raise the fix-up's flag (a run of more than 32), and that no run length close to that limit comes from anything but
exact duplicates - equal m share a key whatever the rounding, near ties may not."""
import numpy as np
import pytest

import sort32_fixtures as F
from oracle import sort32

# longest run of equal keys, by oracle/sort32.py (draws: np.random.default_rng(2) per fixture)
LONGEST_RUN = {
    "gauss_1": 1, "gauss_2": 1, "gauss_3": 1, "gauss_255": 1, "gauss_256": 1, "gauss_257": 1, "gauss_4095": 1,
    "gauss_4096": 1, "gauss_4097": 1, "gauss_70001": 2, "gauss_1048576": 2,
    "dup_x2": 2, "dup_x3": 3, "dup_x31": 31, "dup_x32": 32, "dup_x33": 33,
    "run32_after_240": 32, "run32_after_255": 32, "run32_after_4080": 32, "run32_after_4095": 32,
    "run33_after_4080": 33,
    "near_ties": 8, "cluster8": 8, "mixed_run": 12, "grid_20000": 96,
    "mixture_4097": 3, "mixture_70001": 17, "mixture_1048576": 185,
    "wrap": 32,
    "all_equal_32": 32, "all_equal_33": 33, "overflow_12": 12, "overflow_42": 42,
    "inf_22": 22, "inf_plus_only_22": 22, "inf_300": 300,
    "range_1e-290": 1, "denormal_20": 20, "denormal_40": 40,
    "ends": 5, "signed_zeros": 5, "band_edge_runs": 8,
}
FLAGGED = {"dup_x33", "run33_after_4080", "grid_20000", "mixture_1048576", "all_equal_33", "overflow_42", "inf_300",
           "denormal_40"}


def test_every_fixture_is_pinned():
    assert set(LONGEST_RUN) == set(F.NAMES)


@pytest.mark.parametrize("name", F.NAMES)
def test_longest_run_and_flag(name):
    run, flag, order, ms, ids = F.reference(name)
    assert run == LONGEST_RUN[name]
    assert bool(flag) == (name in FLAGGED) == (run > sort32.MAX_RUN)
    # a run length near the limit of 32 must not hinge on how near ties round into keys
    if 30 <= run <= 35:
        assert F.exact(name), name
    m = F.get(name)
    assert np.array_equal(ms.view(np.uint64), m[order].view(np.uint64))
    assert np.all(ms[1:] >= ms[:-1])


def test_key_map_cases():
    k = sort32.keys32
    assert list(k(np.array([0.0, 1.0, 0.5, 0.25]))) == [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x3FFFFFFF]     # truncation
    assert list(k(np.array([3.0, 3.0, 3.0]))) == [0, 0, 0]                       # empty range
    assert not k(F.get("overflow_12")).any()                                     # hi - lo overflows: scale 0
    assert not k(F.get("inf_22")).any() and not k(F.get("inf_plus_only_22")).any()
    assert not k(F.get("denormal_20")).any()                                     # scale overflows: degenerate
    kr = k(F.get("range_1e-290"))
    assert kr.min() == 0 and kr.max() >= 0xFFFFFFFE and len(set(kr.tolist())) == 300    # tiny range, finite scale
    ke = k(F.get("ends"))
    assert (ke == 0xFFFFFFFF).sum() == 5 and (ke == 0).sum() == 4                # the saturated and the zero key
    assert sort32.max_run(np.array([5, 1, 5, 2, 5, 1], dtype=np.uint32)) == 3
    assert sort32.max_run(np.zeros(0, dtype=np.uint32)) == 0


def test_designed_runs_sit_where_the_names_say():
    for p in F.BOUNDARY_P:
        m = F.get(f"run32_after_{p}")
        assert (m < 0.25).sum() == p and (m == 0.25).sum() == 32
        assert p // 256 != (p + 31) // 256                       # across a block of the fix-up
    assert 4080 // 4096 != (4080 + 31) // 4096 and 4095 // 4096 != (4095 + 31) // 4096    # and a tile of the sort
    m = F.get("wrap")
    assert m.size > 16384 * 256 and (m < 3.5).sum() >= 16384 * 256 and (m == 3.5).sum() == 32
    # near ties: stored in descending m by row, one key per cluster (so the stable sort delivers them reversed)
    m, keys = F.get("near_ties"), sort32.keys32(F.get("near_ties"))
    at = 500
    for c in (2, 3, 4, 5, 6, 7, 8):
        assert np.all(np.diff(m[at:at + c]) < 0) and len(set(keys[at:at + c].tolist())) == 1
        at += c
    mm, km = F.get("mixed_run"), sort32.keys32(F.get("mixed_run"))
    run = np.r_[250:256, 506:512]
    assert len(set(km[run].tolist())) == 1 and len(set(mm[run].tolist())) == 4
    # signed zeros: the (m, row) order keeps them in row order; the bit order would not
    order, ms, ids = sort32.expected(F.get("signed_zeros"))
    assert list(order) == [3, 0, 1, 4, 5, 6, 2]
    # band-edge runs: 8 equal values across ranks 800 and 3200 of 4000
    s = np.sort(F.get("band_edge_runs"))
    for e in (800, 3200):
        assert len(set(s[e - 4:e + 4].tolist())) == 1 and s[e - 5] < s[e - 4] and s[e + 3] < s[e + 4]


@pytest.mark.parametrize("case", list(F.REPLICATED_CASES))
def test_replicated_data_runs_along_the_oracle_trajectory(case):
    """every row 32 times: the longest run is 32 in iterations 1 ... 11, the tied groups lie thousands of key spacings
    apart (rounding differences of the device's m cannot merge two); every row 33 times: 33, so every 32-bit attempt
    of the solve is flagged - at iteration 1 and again at iteration 66, when the pause of 64 iterations ends"""
    kw = F.REPLICATED_CASES[case]
    X, y = F.replicated_problem(32)
    for k in range(1, 12):
        m = F.oracle_m(X, y, kw, k)
        assert sort32.max_run(sort32.keys32(m)) == 32, k
        assert sort32.min_gap_in_keys(np.round(m, 12)) > 1000, k
    X, y = F.replicated_problem(33)
    for k in (1, 2, 13, 66):
        assert sort32.max_run(sort32.keys32(F.oracle_m(X, y, kw, k))) == 33, k


@pytest.mark.parametrize("case", list(F.IDENTITY_CASES))
def test_identity_data_runs_along_the_oracle_trajectory(case):
    """the comparison of the two key widths: Gaussian rows give runs of 1 - 3 keys in iterations 1 ... 13 (never a
    redo), the 33-fold rows a run of 33 at iteration 1 (a redo, then the pause)"""
    kw = F.IDENTITY_CASES[case]
    X, y = F.gaussian_problem()
    for k in range(1, 14):
        assert sort32.max_run(sort32.keys32(F.oracle_m(X, y, kw, k))) <= 3, k
    X, y = F.replicated_problem(33)
    assert sort32.max_run(sort32.keys32(F.oracle_m(X, y, kw, 1))) == 33
