"""Every device implementation of the z-step on a PRESCRIBED m against the exact PAV (tests/zstep_inject.py: the
injection through set_state, the patterns, the reference, the thread hub; test_zstep_inject_host.py pins the oracle's
verdicts and runs the same sharded cases on the CPU engine).

    path 1  single handle, 64-bit sort + merge-tree PAV        RBL_NO_ZBAND=1 RBL_NO_SORT32=1      sort_passes 8
    path 2  single handle, 32-bit keys, fix-up, 64-bit redo    RBL_NO_ZBAND=1                      sort_passes 4 / 12
    path 3  single handle, sort-free banded path               RBL_ZBAND_MIN_N=16                  stats.zband 1 / 2
    path 4  row-sharded, sample sort + chunk PAV + seam search  RBL_NO_ZBAND=1, ranks as threads
    path 5  row-sharded, sort-free                             RBL_ZBAND_MIN_N=16, ranks as threads

Value: max |z - z_exact| <= 1e-10 max(1, max |z_exact|) on every path (the bar of test_pav_vs_oracle).  Path: keys tied
across a band edge are never certified; of the cases the oracle certifies at most a quarter per family may be redone,
each printed with its status word.  Every figure is printed before it is asserted (pytest -s)."""
import pathlib

import numpy as np
import pytest

from oracle import sort32, zband

import zstep_inject as Z

GOLDEN = pathlib.Path(__file__).parent / "golden"
pytestmark = pytest.mark.gpu

ENV = {"sort64": {"RBL_NO_ZBAND": "1", "RBL_NO_SORT32": "1"}, "sort32": {"RBL_NO_ZBAND": "1", "RBL_NO_SORT32": "0"},
       "banded": {"RBL_NO_ZBAND": "0", "RBL_NO_SORT32": "0", "RBL_ZBAND_MIN_N": "16"}}
HANDLES = {}                      # (path, family, loss, n) -> [solver, next iteration number]
CERT = {}                         # (path 3 or 5, family) -> [oracle-OK cases certified, redone]
SPLIT = [0, 0]                    # path 3: certified steps, those with a block valued from bracket-split sums


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    yield rbl
    for s, _ in HANDLES.values():
        s.close()
    HANDLES.clear()


def _setenv(monkeypatch, path):
    for k, v in ENV[path].items():
        monkeypatch.setenv(k, v)


def _handle(R, monkeypatch, path, fam, loss, n, fresh=False):
    """the shared handle of (path, family, loss, n); the environment is read at its first z-step, run here"""
    key = (path, fam, loss, n)
    if fresh or key not in HANDLES:
        _setenv(monkeypatch, path)
        s = Z.make_solver(R, fam, loss, n)
        Z.inject(s, Z.pattern("gaussian", n, 99, fam), 1.0, 1)
        if fresh:
            return [s, 200]
        HANDLES[key] = [s, 200]
    return HANDLES[key]


def _step(h, path, fam, loss, m0, rho, it=None, peek=False, label=""):
    """one injected iteration, value and path checked -> the result of Z.inject plus err / verdict"""
    s = h[0]
    if it is None:
        it, h[1] = h[1], h[1] + 100          # past any pause (<= 64 iterations) left by the step before
    r = Z.inject(s, m0, rho, it, peek=peek)
    assert np.array_equal(r["m"], m0), (label, "m was not injected exactly")
    zref = Z.exact_z(fam, loss, rho, r["m"])
    r["err"], r["zref"] = Z.value_error(r["z"], zref), zref
    r["verdict"] = Z.verdict(fam, loss, rho, r["m"])[0] if path == "banded" else None
    print(f"{label} {path} {fam} {loss[:6]} n={m0.size} rho=2^{int(np.log2(rho))} iter={it}: err={r['err']:.2e} "
          f"mode={r['mode']} passes={r['passes']} status={r['status']} split={r['split']} oracle={r['verdict']}")
    assert r["err"] <= Z.BAR, (label, path, fam, loss, m0.size, rho, it, r["err"], r["mode"], r["passes"], r["status"])
    return r


def _check_path(r, path, fam, paused=False):
    n = r["m"].size
    if path == "sort64" or paused:
        assert r["mode"] == 0 and r["passes"] == 8, (r["mode"], r["passes"])
    elif path == "sort32":
        assert r["mode"] == 0 and r["passes"] == (12 if sort32.flagged(r["m"]) else 4), (r["mode"], r["passes"])
    else:
        assert r["mode"] in (0, 1, 2)
        if r["mode"] == 1:
            SPLIT[0] += 1
            SPLIT[1] += r["split"] != 0
        if r["verdict"] == zband.TIE:
            assert r["mode"] == 2 and r["status"] != 0, ("keys tied across a band edge were certified", r["mode"], r["status"])
        elif r["verdict"] == zband.OK:
            assert r["mode"] in (1, 2)
            c = CERT.setdefault((3, fam), [0, 0])
            c[r["mode"] - 1] += 1
            if r["mode"] == 2:
                print(f"   oracle-OK case redone with the sort: n={n} status word {r['status']}")


def _run_single(R, monkeypatch, path, fam, loss, n, names):
    h = _handle(R, monkeypatch, path, fam, loss, n)
    for k, (m0, rho, _) in enumerate(Z.injections(fam, n, names)):
        r = _step(h, path, fam, loss, m0, rho, label=str(names[k]))
        _check_path(r, path, fam)


def _ids(cases):
    return [f"{c[0]}-{c[1][:6]}-{c[2]}-{k}" for k, c in enumerate(cases)]


# ------------------------------------------------------------------------------------------------ value and path
@pytest.mark.parametrize("path", ["sort64", "sort32"])
@pytest.mark.parametrize("fam,loss,n,names", Z.SINGLE_SORT, ids=_ids(Z.SINGLE_SORT))
def test_sorted_paths_on_prescribed_m(R, monkeypatch, path, fam, loss, n, names):
    _run_single(R, monkeypatch, path, fam, loss, n, names)


@pytest.mark.parametrize("fam,loss,n,names", Z.SINGLE_BANDED, ids=_ids(Z.SINGLE_BANDED))
def test_banded_path_on_prescribed_m(R, monkeypatch, fam, loss, n, names):
    _run_single(R, monkeypatch, "banded", fam, loss, n, names)


def test_iteration_zero_takes_the_64_bit_sort(R, monkeypatch):
    """iter = 0 on handles whose fast paths are on: the sort with 64-bit keys, whatever m is"""
    for path, fam in (("sort32", "extremile"), ("banded", "superq_0.5")):
        h = _handle(R, monkeypatch, path, fam, Z.BCE, 6000)
        r = _step(h, path, fam, Z.BCE, Z.pattern("gaussian", 6000, 5, fam), 2.0 ** -4, it=0)
        _check_path(r, path, fam, paused=True)


# --------------------------------------------------------------------------------------------- regression: mid-read
@pytest.mark.parametrize("path,fam,name", [("banded", "superq_0.5", "tie_1000"), ("banded", "aorr_0.2_0.8", "all_equal"),
                                           ("sort32", "extremile", "tight")])
def test_get_state_mid_iteration_settles_an_uncertified_z_step(R, monkeypatch, path, fam, name):
    """rbl_get_state between rbl_phase_z and rbl_phase_q on a step the fast path cannot certify (keys tied across a band
    edge; a run of more than 32 equal 32-bit keys): the read has to settle the verdict and hand out the redone z.  It
    used to return the buffer as the uncertified step left it (the z of the iteration before, or one sorted with a
    broken run): rbl_get_state did not pass through the entry that settles, while DESIGN.md said it did - an overridden
    w_subproblem that looks at z would have worked on a stale vector.  The inputs are kept in
    tests/golden/zstep_midread_4096.npz (the sort32 case: a tight cluster and one far value, so that the cluster's distinct
    m share one 32-bit key and their order matters)."""
    n = 4096
    h = _handle(R, monkeypatch, path, fam, Z.BCE, n, fresh=True)
    for rho in (2.0 ** -12, 1.0):
        m0 = np.load(GOLDEN / "zstep_midread_4096.npz")[f"{fam}__{name}"]
        assert m0.shape == (n,)
        r = _step(h, path, fam, Z.BCE, m0, rho, peek=True, label="mid-read")
        if path == "banded":
            assert r["verdict"] == zband.TIE and r["mode"] == 2
        else:
            assert sort32.flagged(m0) and r["passes"] == 12
        err = Z.value_error(r["zmid"], r["zref"])
        print(f"   z read after the z-step: err={err:.2e}")
        assert err <= Z.BAR, err
        assert np.array_equal(r["zmid"], r["z"])
    h[0].close()


# ------------------------------------------------------------------------------------------- stale and exact hints
@pytest.mark.parametrize("fam,loss", [("superq_0.5", Z.BCE), ("aorr_0.2_0.8", Z.HINGE), ("aorr_dc", Z.SQ)])
def test_unrelated_then_repeated_m_on_one_handle(R, monkeypatch, fam, loss):
    """root pass 1 packs its candidates around a prediction from the last three block values: a sequence of unrelated m
    (pattern, scale, shift) makes every prediction stale, the same m three times makes it exact.

    Regression: aorr [0.2, 0.8] / hinge used to give a third repeat that differed from the first two in 14 of 6000
    entries by one ulp (max |z_3 - z_1| = 5.6e-17): the pooled block's sums were split between the root pass's frozen
    part and the gathered elements, the split followed the bracket and the bracket followed the hint.  k_zb_canon now
    takes the block value from sums over the certified block alone."""
    n = 6000
    h = _handle(R, monkeypatch, "banded", fam, loss, n, fresh=True)
    seq = [("gaussian", 1.0, 0.0), ("wide", 1.0, 0.0), ("sorted", 2.0 ** -10, 3.0), ("reversed", 2.0 ** 6, -40.0),
           ("one_shard_large", 2.0 ** -3, -1.0), ("gaussian", 2.0 ** 10, 0.0), ("sorted", 1.0, -1.0)]
    it = 300
    for k, (name, scale, shift) in enumerate(seq):
        m0 = Z.pattern(name, n, 11 + k, fam, scale=scale, shift=shift)
        r = _step(h, "banded", fam, loss, m0, Z.RHOS[(k + 1) % 4], it=it, label=f"stale {name}")
        _check_path(r, "banded", fam)
        it += 1 if r["mode"] == 1 else 100
    m0 = Z.pattern("gaussian", n, 31, fam, shift=0.5)
    zs = []
    for k in range(3):
        r = _step(h, "banded", fam, loss, m0, 2.0 ** -4, it=it, label="repeat")
        _check_path(r, "banded", fam)
        assert r["mode"] == 1                        # (oracle-OK, and certified: the consecutive iterations below need it)
        assert r["split"] == 0, "a block value came from bracket-split sums: it may follow the hint"
        zs.append(r["z"])
        it += 1
    print("   repeated m: max |z_k - z_0| =", [float(np.max(np.abs(z - zs[0]))) for z in zs[1:]],
          "entries that differ:", [int(np.count_nonzero(z != zs[0])) for z in zs[1:]])
    assert np.array_equal(zs[0], zs[1]) and np.array_equal(zs[1], zs[2])
    h[0].close()


def test_block_value_followed_the_hint_regression(R, monkeypatch):
    """tests/golden/zstep_repeat_aorr_hinge_6000.npy: three unrelated m (rows 0-2) and one m (row 3) that is then given
    three times, aorr [0.2, 0.8] / hinge, n = 6000, certified iterations 304 ... 309.  The third repeat used to differ
    from the first two in 14 entries by one ulp: the block value came from sums split between a root pass's frozen part
    and the gathered elements, the split followed the bracket and the bracket the hint (exact after two repeats)."""
    fam, loss = "aorr_0.2_0.8", Z.HINGE
    rows = np.load(GOLDEN / "zstep_repeat_aorr_hinge_6000.npy")
    assert rows.shape == (4, 6000)
    h = _handle(R, monkeypatch, "banded", fam, loss, 6000, fresh=True)
    zs = []
    for k, j in enumerate((0, 1, 2, 3, 3, 3)):
        rho = Z.RHOS[(k + 5) % 4] if k < 3 else 2.0 ** -4
        r = _step(h, "banded", fam, loss, rows[j].copy(), rho, it=304 + k, label="hint regression")
        assert r["mode"] == 1 and r["split"] == 0, (k, r["mode"], r["status"], r["split"])
        if k >= 3:
            zs.append(r["z"])
    print("   max |z_k - z_0| =", [float(np.max(np.abs(z - zs[0]))) for z in zs[1:]])
    assert np.array_equal(zs[0], zs[1]) and np.array_equal(zs[1], zs[2])
    h[0].close()


# ------------------------------------------------------------------------------------------------------- back-off
def test_banded_back_off_doubles_caps_and_resets(R, monkeypatch):
    fam, loss, n = "superq_0.5", Z.BCE, 4096
    h = _handle(R, monkeypatch, "banded", fam, loss, n, fresh=True)
    tie, good = Z.pattern("all_equal", n, 1, fam), Z.pattern("gaussian", n, 2, fam)

    def step(m0, it, want):
        r = _step(h, "banded", fam, loss, m0, 2.0 ** -4, it=it, label=f"back-off want {want}")
        assert r["mode"] == want, (it, r["mode"], want, r["status"])

    step(good, 10, 1)
    it = 11
    for pause in (2, 4, 8, 16, 32, 64, 64, 64):
        step(tie, it, 2)                             # not certified: the path pauses until it + 1 + pause
        step(good, it + 1, 0)
        step(tie, it + pause, 0)                     # the last paused iteration: the sort, whatever m is
        it = it + 1 + pause
    step(good, it, 1)                                # resumes on a benign m; a certified step resets the pause
    step(tie, it + 1, 2)
    step(good, it + 3, 0)
    step(good, it + 4, 1)
    h[0].close()


def test_sort32_pauses_64_iterations_after_a_redo(R, monkeypatch):
    fam, loss, n = "extremile", Z.BCE, 4096
    h = _handle(R, monkeypatch, "sort32", fam, loss, n, fresh=True)
    grid, good = Z.pattern("two_values", n, 1, fam), Z.pattern("gaussian", n, 2, fam)
    assert sort32.flagged(grid) and not sort32.flagged(good)
    for it, m0, want in ((10, good, 4), (11, grid, 12), (12, good, 8), (75, grid, 8), (76, good, 4), (77, grid, 12),
                         (141, good, 8), (142, good, 4)):
        r = _step(h, "sort32", fam, loss, m0, 2.0 ** -4, it=it, label=f"s32 pause want {want}")
        assert r["passes"] == want and r["mode"] == 0, (it, r["passes"], want)
    h[0].close()


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("path,fam,loss,name", [("sort64", "esrm", Z.HINGE, "wide"), ("sort32", "extremile", Z.BCE, "gaussian"),
                                                ("sort32", "ehrm", Z.BCE, "grid"), ("banded", "aorr_0.2_0.8", Z.BCE, "gaussian"),
                                                ("banded", "superq_0.37", Z.SQ, "tie_3000")])
def test_single_handle_gives_the_same_bits_twice(R, monkeypatch, path, fam, loss, name):
    n, zs = 6000, []
    for _ in range(2):
        h = _handle(R, monkeypatch, path, fam, loss, n, fresh=True)
        r = _step(h, path, fam, loss, Z.pattern(name, n, 3, fam), 2.0 ** -12, label="twice")
        zs.append((r["z"], r["mode"], r["passes"]))
        h[0].close()
    assert zs[0][1:] == zs[1][1:] and np.array_equal(zs[0][0], zs[1][0])


# --------------------------------------------------------------------------------------------------- sharded paths
def _run_sharded(monkeypatch, fam, loss, n, names, world, banded):
    import torch  # noqa: F401  (imports finish in this thread before the rank threads start)
    import admm_for_rank_based_loss_amd as rbl
    from admm_for_rank_based_loss_amd import dist as _d  # noqa: F401
    rbl._lib.load()
    _setenv(monkeypatch, "banded" if banded else "sort32")
    inj = Z.injections(fam, n, names)
    res = Z.run_sharded(Z.GpuRank, fam, loss, n, world, banded, inj)
    seen = Z.check_sharded(fam, loss, res, inj, banded, f"w{world}")
    Z.check_chunks(names, res, n, world)
    return inj, res, seen


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("fam,loss,n,names", Z.SHARDED_SORT, ids=_ids(Z.SHARDED_SORT))
def test_sharded_sort_path_on_prescribed_m(R, monkeypatch, fam, loss, n, names, world):
    """path 4; a seam search that does not finish within its rounds raises out of the rank's step"""
    inj, res, seen = _run_sharded(monkeypatch, fam, loss, n, names, world, False)
    for r in res:
        assert all(rec["mode"] == 0 for rec in r["recs"])
    for nm, (m0, rho, _), r in zip(names, inj, res):
        if fam == "extremile" and isinstance(nm, tuple) and rho == 2.0 ** -20:
            # the input meant to pool into ONE block over all ranks does (the exact z is constant), and so does the device's
            assert np.ptp(Z.exact_z(fam, loss, rho, r["m"])) == 0.0
            assert np.ptp(r["z"]) <= Z.BAR * max(1.0, abs(r["z"][0])), np.ptp(r["z"])


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("fam,loss,n,names", Z.SHARDED_BANDED, ids=_ids(Z.SHARDED_BANDED))
def test_sharded_banded_path_on_prescribed_m(R, monkeypatch, fam, loss, n, names, world):
    """path 5: _z_banded() returns the same verdict on every rank, False on tied keys; the redone z is checked too"""
    inj, res, seen = _run_sharded(monkeypatch, fam, loss, n, names, world, True)
    for (st, certified), r in zip(seen, res):
        rec = r["recs"][0]
        assert rec["mode"] == 1 if certified else rec["mode"] in (0, 2), rec
        if st == zband.OK:
            c = CERT.setdefault((5, fam), [0, 0])
            c[0 if certified else 1] += 1
            if not certified:
                print(f"   oracle-OK case redone with the sort: n={n} world={world} status word {rec['status']}")


@pytest.mark.parametrize("banded,fam,loss", [(False, "extremile", Z.BCE), (True, "aorr_0.2_0.8", Z.HINGE)])
def test_sharded_paths_give_the_same_bits_twice(R, monkeypatch, banded, fam, loss):
    zs = [_run_sharded(monkeypatch, fam, loss, 4099, ["gaussian", "reversed"], 3, banded)[1] for _ in range(2)]
    for a, b in zip(*zs):
        assert np.array_equal(a["z"], b["z"])


# ------------------------------------------------------------------------------------------------------- the cap
def test_fast_path_certifies_what_the_oracle_certifies(R, monkeypatch):
    """at most a quarter of the oracle-OK cases per family come back redone: the file does not silently test the sort
    alone.  (Run on its own, the test first runs the benign patterns of every banded family.)"""
    for fam in Z.BANDED:
        if (3, fam) not in CERT:
            _run_single(R, monkeypatch, "banded", fam, Z.HINGE, 6000, Z.BENIGN)
        if (5, fam) not in CERT:
            for st, certified in _run_sharded(monkeypatch, fam, Z.HINGE, 6000, Z.BENIGN, 2, True)[2]:
                if st == zband.OK:
                    CERT.setdefault((5, fam), [0, 0])[0 if certified else 1] += 1
    print({key: tuple(c) for key, c in CERT.items()})
    print(f"path 3: {SPLIT[0]} certified steps, {SPLIT[1]} with a block valued from bracket-split sums")
    for path in (3, 5):
        for fam in Z.BANDED:
            ok, redone = CERT[(path, fam)]
            assert ok + redone > 0 and 4 * redone <= ok + redone, (path, fam, ok, redone)
