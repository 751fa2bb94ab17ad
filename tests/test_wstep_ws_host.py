"""The working-set lasso (l1_solver="working_set": RBL_CREATE_WORKING_SET on a gram="none" handle) without a GPU: the
fixtures of tests/test_gpu_wstep_ws.py recomputed by an independent solver (KKT-tight, positive definite active block,
support where the case needs it), the NumPy restatement of the loop (tests/wstep_ws_ref.py) on them, its selection order
against a brute-force statement of the rule, the public header, the Python refusals - raised before any device call -
and the bookkeeping header replayed under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import wstep_op_ref as opref
import wstep_ws_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rbl.h")).read()
KKT = 1e-9
# the issue's table: support, smallest / largest eigenvalue of the active block at kappa = 0.05 max|q|
TABLE = {(500, 2047): (41, 1.40, 501), (500, 2048): (43, 1.35, 501), (500, 2049): (41, 1.74, 501),
         (500, 4097): (32, 1.46, 500), (3000, 16385): (77, 2.06, 3000), (3000, 20000): (64, 2.75, 3000)}


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


@pytest.fixture(scope="module")
def solved():
    """(n, d) -> (D, q, reg, w of the independent solver), computed once"""
    out = {}
    for n, d in ref.SHAPES:
        A, q = ref.fixture(n, d)
        reg = 2 * ref.RHO * ref.KAPPA_FRAC * float(np.max(np.abs(q)))
        out[(n, d)] = (A, q, reg, ref.independent_lasso(A, q, ref.RHO, reg=reg))
    return out


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_fixture_supports_are_where_the_gpu_cases_need_them(solved, shape):
    """a fixture that drifts fails here, on the CPU: the independent solution is KKT-tight, its active block positive
    definite, and its support the issue's (<= 80: the active-set kernel's cases)"""
    A, q, reg, w = solved[shape]
    qm = float(np.max(np.abs(q)))
    kkt = opref.enet_kkt(A, q, ref.RHO, reg, None, w)
    lo, hi = ref.active_block_eigs(A, w, ref.RHO)
    sup = int(np.count_nonzero(w))
    print(f"{shape}: support {sup}, KKT residual {kkt:.3e}, active block eigenvalues {lo:.3f} .. {hi:.1f}")
    assert kkt <= 1e-11 * max(1.0, qm)
    want = TABLE[shape]
    assert sup == want[0] and sup <= 80 < ref.FS_MAX
    assert lo == pytest.approx(want[1], abs=0.006) and hi == pytest.approx(want[2], abs=1.0) and lo > 1.0


def test_overflow_fixture_is_past_the_active_set_kernel():
    """500 x 4097 at kappa = 0.03 max|q|: pure l1 has 114 active coordinates, with l2_j in rho [0.5, 2] still > 96"""
    n, d, frac = ref.OVERFLOW
    A, q = ref.fixture(n, d)
    qm = float(np.max(np.abs(q)))
    reg = 2 * ref.RHO * frac * qm
    w = ref.independent_lasso(A, q, ref.RHO, reg=reg)
    assert np.count_nonzero(w) == 114 and opref.enet_kkt(A, q, ref.RHO, reg, None, w) <= 1e-11 * qm
    l1, l2 = np.full(d, reg), ref.overflow_l2(d)
    assert np.all((l2 >= 0.5 * ref.RHO) & (l2 <= 2.0 * ref.RHO))
    w = ref.independent_lasso(A, q, ref.RHO, l1=l1, l2=l2)
    assert np.count_nonzero(w) > ref.FS_MAX and opref.enet_kkt(A, q, ref.RHO, l1, l2, w) <= 1e-11 * qm
    assert ref.active_block_eigs(A, w, ref.RHO, l2)[0] > 0.5


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_restated_loop_ends_kkt_tight_on_every_fixture(solved, shape):
    A, q, reg, w_ind = solved[shape]
    qm = float(np.max(np.abs(q)))
    w, rep = ref.working_set_lasso(A, q, ref.RHO, reg=reg, tol=1e-13)
    assert not rep["left_route"] and rep["evictions"] == 0
    assert opref.enet_kkt(A, q, ref.RHO, reg, None, w) <= KKT * max(1.0, qm)
    assert np.array_equal(w != 0, w_ind != 0)
    assert np.max(np.abs(w - w_ind)) <= 1e-10 * max(1.0, float(np.max(np.abs(w_ind))))
    # at most one column per chunk and round: the rounds say so
    assert rep["rows_last"] <= rep["rounds"] * min(ref.SELECT, -(-A.shape[1] // ref.CHUNK))


def test_restated_loop_elastic_net_free_coordinate_capacity_and_sequence():
    A, q = ref.fixture(500, 4097)
    d = A.shape[1]
    qm = float(np.max(np.abs(q)))
    rng = np.random.default_rng(d + 1)
    l1 = 2 * ref.RHO * 0.05 * qm * rng.uniform(0.5, 2.0, d)
    l1[d - 1] = 0.0
    l2 = ref.RHO * rng.uniform(0.5, 2.0, d)
    w, rep = ref.working_set_lasso(A, q, ref.RHO, l1=l1, l2=l2)
    assert w[d - 1] != 0.0 and not rep["left_route"]
    assert opref.enet_kkt(A, q, ref.RHO, l1, l2, w) <= KKT * qm
    w_ind = ref.independent_lasso(A, q, ref.RHO, l1=l1, l2=l2)
    assert np.array_equal(w != 0, w_ind != 0) and np.max(np.abs(w - w_ind)) <= 1e-10 * np.max(np.abs(w_ind))
    # a capacity below the support: the loop evicts what it can and then gives up
    w2, rep2 = ref.working_set_lasso(A, q, ref.RHO, l1=l1, l2=l2, cap=16)
    assert rep2["left_route"] == 1 and np.count_nonzero(w2) <= 16
    # a sequence on one working set: Gs only grows, and an unchanged support forms no row
    st = {}
    b2 = np.random.default_rng(11).standard_normal(A.shape[0])
    formed = []
    for k in range(5):
        qk = q + 0.01 * k * (A.T @ b2)
        w, rep = ref.working_set_lasso(A, qk, ref.RHO, l1=l1, l2=l2, w0=w if k else None, state=st)
        formed.append(rep["rows_last"])
        assert opref.enet_kkt(A, qk, ref.RHO, l1, l2, w) <= KKT * qm
    assert all(f < len(st["S"]) // 4 for f in formed[1:]), formed
    w_again, rep = ref.working_set_lasso(A, qk, ref.RHO, l1=l1, l2=l2, w0=w, state=st)
    assert rep["rows_last"] == 0 and rep["rounds"] == 1 and np.array_equal(w_again != 0, w != 0)


def _prescribed(ld, seed):
    """g, kappa, member, q with ties within and across chunks, a chunk of no candidates, a candidate in the last column
    and a free coordinate (kappa = 0)"""
    rng = np.random.default_rng(seed)
    g = np.round(rng.standard_normal(ld) * 4.0) / 4.0       # quarter steps: many exact ties
    kappa = np.full(ld, 0.75)
    member = rng.random(ld) < 0.05
    q = rng.standard_normal(ld)
    nchunks = -(-ld // ref.CHUNK)
    if nchunks > 2:
        g[ref.CHUNK:2 * ref.CHUNK] = 0.5                    # chunk 1: |g| below kappa everywhere - no candidate
    g[ld - 1], member[ld - 1] = -9.0, False                 # the last column: the largest violation of its chunk
    g[7], g[ref.CHUNK // 2] = 5.0, -5.0                     # a tie inside chunk 0: column 7 wins
    member[7] = member[ref.CHUNK // 2] = False
    kappa[3], g[3], member[3] = 0.0, 4.0, False             # a free coordinate: |g| itself is its violation (4 < 5 - 0.75)
    return g, kappa, member, q


@pytest.mark.parametrize("ld", [2048, 2050, 4098, 6 * 2048 + 2])
def test_selection_order_is_the_brute_force_rule(ld):
    g, kappa, member, q = _prescribed(ld, ld)
    for d in (ld, ld - 1):
        for take in (ref.SELECT, 2, 1):
            got = ref.select(g, kappa, member, d, q, 1e-13, take)
            assert got == ref.select_brute(g, kappa, member, d, q, 1e-13, take)
    got = ref.select(g, kappa, member, ld, q, 1e-13)
    assert got[0] == ld - 1 and ref.CHUNK // 2 not in got and 3 not in got
    assert (7 in got) == (ld > ref.CHUNK)                   # one winner per chunk: at ld = 2048 the last column is chunk 0's
    if ld > 2 * ref.CHUNK:
        assert all(not (ref.CHUNK <= j < 2 * ref.CHUNK) for j in got)
    assert len(got) == len({j // ref.CHUNK for j in got})
    # ties across chunks: equal violations come out in column order
    g2, k2, m2 = np.zeros(ld), np.full(ld, 0.5), np.zeros(ld, dtype=bool)
    g2[[5, ld - 2]] = 2.0
    assert ref.select(g2, k2, m2) == ([5, ld - 2] if ld > ref.CHUNK else [5]) == ref.select_brute(g2, k2, m2)
    # nothing above the threshold, and a threshold that max|q| raises above every violation
    assert ref.select(np.full(ld, 0.5), k2, m2) == [] == ref.select_brute(np.full(ld, 0.5), k2, m2)
    assert ref.select(g2, k2, m2, q=np.full(ld, 1e3), tol=1e-2) == []
    # every column a member
    assert ref.select(g, kappa, np.ones(ld, dtype=bool)) == []


def test_dense_exact_solver_against_the_kkt_conditions():
    rng = np.random.default_rng(2)
    for m in (1, 5, 40):
        B = rng.standard_normal((3 * m, m))
        G = B.T @ B
        q = rng.standard_normal(m) * 3.0
        kap = rng.uniform(0.2, 2.0, m)
        kap[0] = 0.0
        w = ref.dense_lasso_exact(G, q, kap, rng.standard_normal(m) * (rng.random(m) < 0.5))
        g = G @ w - q
        r = np.where(w != 0, g + kap * np.sign(w), np.sign(g) * np.maximum(np.abs(g) - kap, 0.0))
        assert np.max(np.abs(r)) <= 1e-11 * max(1.0, np.max(np.abs(q)))


# ---------------------------------------------------------------------------------------------------- header, binding, Python
def test_header_declares_the_flag_the_report_and_the_entries():
    assert re.search(r"#define\s+RBL_VERSION\s+106\b", HEADER)
    assert re.search(r"#define\s+RBL_CREATE_NO_GRAM\s+1\b", HEADER) and re.search(r"#define\s+RBL_CREATE_WORKING_SET\s+2\b", HEADER)
    for name in ("rbl_wset_info", "rbl_k_wset_gram", "rbl_k_wset_scan", "rbl_k_wstep_ws"):
        assert re.search(r"int\s+%s\(" % name, HEADER), name
    assert "5 = the working set" in HEADER and "4 = the operator route" in HEADER
    assert "the exact active-set kernel needs G and is not used)" not in HEADER        # the amended comment
    assert HEADER.count("src/util/fast_lasso.py") >= 2
    body = re.search(r"typedef struct rbl_wset_report \{(.*?)\} rbl_wset_report;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int64_t|int32_t)\s+([^;]+);", body) for n in decl.split(",")]
    lib = _pkg()._lib
    assert names == [f[0] for f in lib.RblWsetReport._fields_]
    assert set(("rbl_wset_info", "rbl_k_wset_gram", "rbl_k_wset_scan", "rbl_k_wstep_ws")) <= set(lib.SIGNATURES)
    assert (lib.CREATE_NO_GRAM, lib.CREATE_WORKING_SET, lib.WS_CAP, lib.WS_SELECT) == (1, 2, ref.CAP, ref.SELECT)
    plan = open(os.path.join(ROOT, "admm-for-rank-based-loss_amd", "csrc", "wset_plan.h")).read()
    assert re.search(r"WS_CAP = %d;" % ref.CAP, plan) and re.search(r"WS_SELECT = %d;" % ref.SELECT, plan)
    assert "hip" not in plan.lower().replace("wstep_ws.hip", "").replace("(no hip)", "")   # plain C++


def test_l1_solver_resolves_to_the_create_flags():
    s, L = _pkg()._solver, _pkg()._lib
    assert s.resolve_l1_solver("fista", True, "csr", "none") == 0           # today's flags: the default changes nothing
    assert s.resolve_l1_solver("fista", False, "f32", "dense") == 0
    assert s.resolve_l1_solver("working_set", True, "csr", "none") == L.CREATE_WORKING_SET
    with pytest.raises(ValueError, match="l1_solver must be one of"):
        s.resolve_l1_solver("cd", True, "csr", "none")
    with pytest.raises(ValueError, match="needs l1_reg or l1_weights"):
        s.resolve_l1_solver("working_set", False, "csr", "none")
    with pytest.raises(ValueError, match=r'needs storage="csr"'):
        s.resolve_l1_solver("working_set", True, "f64", "dense")
    with pytest.raises(ValueError, match=r'needs gram="none"'):
        s.resolve_l1_solver("working_set", True, "csr", "dense")
    import inspect
    for cls in (_pkg().ADMMmethod, _pkg().OneVsRest, s.Solver):
        assert inspect.signature(cls.__init__).parameters["l1_solver"].default == "fista", cls
    assert "l1_solver" in _pkg().ADMMgroup._KEYS
    assert "l1_solver" not in inspect.signature(_pkg().smoothADMMmethod.__init__).parameters
    assert list(inspect.signature(_pkg().ADMMmethod.__init__).parameters)[-1] == "share_data"


def _xy(d=12, n=30):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, d))
    X[np.abs(X) < 0.8] = 0.0
    return X, np.where(rng.standard_normal(n) > 0, 1.0, -1.0)


def test_python_refusals_come_before_any_device_call(monkeypatch):
    rbl = _pkg()

    def boom():
        raise AssertionError("the library was loaded: a device call was about to be made")

    monkeypatch.setattr(rbl._lib, "load", boom)
    X, y = _xy()
    A = sp.csr_matrix(X)
    kw = dict(weight_function="erm", loss="binary_cross_entropy")
    with pytest.raises(ValueError, match="needs l1_reg or l1_weights"):
        rbl.ADMMmethod(A, y, l2_reg=0.1, storage="csr", gram="none", l1_solver="working_set", **kw)
    with pytest.raises(ValueError, match="needs l1_reg or l1_weights"):
        rbl.ADMMmethod(A, y, l2_weights=np.full(12, 0.1), storage="csr", gram="none", l1_solver="working_set", **kw)
    with pytest.raises(ValueError, match=r'l1_solver="working_set" needs storage="csr"'):
        rbl.ADMMmethod(X, y, l1_reg=0.1, storage="f64", l1_solver="working_set", **kw)
    with pytest.raises(ValueError, match=r'l1_solver="working_set" needs gram="none"'):
        rbl.ADMMmethod(A, y, l1_reg=0.1, storage="csr", gram="dense", l1_solver="working_set", **kw)
    with pytest.raises(ValueError, match=r'l1_solver="working_set" needs gram="none"'):
        rbl.ADMMmethod(A, y, l1_reg=0.1, storage="csr", l1_solver="working_set", **kw)       # "auto" at d = 12 is "dense"
    with pytest.raises(ValueError, match="l1_solver must be one of"):
        rbl.ADMMmethod(A, y, l1_reg=0.1, storage="csr", gram="none", l1_solver="exact", **kw)
    with pytest.raises(TypeError, match="l1_solver"):
        rbl.smoothADMMmethod(A, y, l1_reg=0.1, storage="csr", l1_solver="working_set", **kw)
    with pytest.raises(ValueError, match=r'l1_solver="working_set" needs gram="none"'):
        rbl.OneVsRest(A, np.arange(X.shape[0]) % 3, l1_reg=0.1, storage="csr", gram="dense", l1_solver="working_set")
    with pytest.raises(ValueError, match="problem 1: l1_solver must be the same for every problem"):
        rbl.ADMMgroup(A, y, [dict(l1_reg=0.1, gram="none", l1_solver="working_set"), dict(l1_reg=0.2, gram="none")], storage="csr")
    with pytest.raises(ValueError, match="problem 0: l1_solver must be one of"):
        rbl.ADMMgroup(A, y, [dict(l1_reg=0.1, gram="none", l1_solver=1)], storage="csr")
    with pytest.raises(ValueError, match="problem 0: .*needs l1_reg or l1_weights"):
        rbl.ADMMgroup(A, y, [dict(l2_reg=0.1, gram="none", l1_solver="working_set")], storage="csr")
    with pytest.raises(ValueError, match=r'problem 0: l1_solver="working_set" needs storage="csr"'):
        rbl.ADMMgroup(X, y, [dict(l1_reg=0.1, l1_solver="working_set")], storage="f32")


def test_bookkeeping_program_passes_under_the_sanitizers(tmp_path):
    """S, pos, the rows of Gs that are owed, eviction and compaction replayed against a dense model - refusals, a free
    coordinate that stays with w = 0, an evicted column that comes back, filling to WS_CAP at ld = 20 004"""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wset_plan_main")
    src = os.path.join(ROOT, "tests", "wset_plan_main.cpp")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and ("cannot find" in cc.stderr or "unsupported" in cc.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "wset_plan: ok" in run.stdout, run.stdout + run.stderr
