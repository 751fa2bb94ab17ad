"""An input replaced between two iterations (csrc/derived_state.h: one cause per entry point): the handle goes on exactly as
a fresh handle does that is given the same data and the same state.  Every solve runs with tol = 0, so nothing converges,
and the twin runs the same kernels as the handle under test: the bar is bit equality of w, z, lambda, rho and of the
fused / mispredicted / fused_v figures, step by step.  Shapes: the narrowest rows that have a single-sweep erm pass
(more than 32 packets per row: d = 132 in float32, d = 68 in float64), n = 1536 - three blocks of rows and a tail.

On the parent of the commit that added this module (flags cleared by hand per entry point) the erm cases failed:
  * upload between fused iterations - the stale z_next / q of the old D were swapped in and D^T lambda never re-seeded;
  * the same under a borrower, which also kept the owner's old Lipschitz bound;
  * finalize_smooth - z_next / q of the un-thresholded w were swapped in."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BCE, HINGE = "binary_cross_entropy", "hinge"
N = 1536
WIDTH = {"f32": 132, "f64": 68}


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


_problems = {}


def _problem(n, d, seed):
    """computed once per shape and seed, shared, never written to"""
    if (n, d, seed) not in _problems:
        from oracle import problems
        X, y = problems.make_problem(n, d, seed=seed)
        X.setflags(write=False)
        _problems[(n, d, seed)] = (X, np.asarray(y, dtype=np.float64).reshape(-1))
    return _problems[(n, d, seed)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _steps(s, k):
    """k iterations -> per step (fused, mispredicted, fused_v, rho, iter, bits of w, z, lambda)"""
    out = []
    for _ in range(k):
        st = s.step(False)
        g = s.get_state()
        out.append((st.fused, st.mispredicted, st.fused_v, g["rho"], g["iter"], _bits(g["w"]), _bits(g["z"]), _bits(g["lam"])))
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[:5] == y[:5], (k, x[:5], y[:5])
        for name, u, v in zip(("w", "z", "lam"), x[5:], y[5:]):
            assert np.array_equal(u, v), (k, name, int(np.sum(u != v)))


def _seed(twin, state):
    twin.set_state(w=state["w"], z=state["z"], lam=state["lam"], rho=state["rho"], iter=state["iter"], smooth_t=state["smooth_t"])


def _fresh(R, X, y, d, kw):
    s = R.Solver(X.shape[0], d, "erm", **kw)
    s.set_data(X, y)
    s.gram()
    return s


# ------------------------------------------------------------------------------- 1. upload between fused iterations
@pytest.mark.parametrize("wstep", ["L1", "L2"])
@pytest.mark.parametrize("loss", [BCE, HINGE])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_upload_between_fused_iterations(R, storage, loss, wstep):
    """four single-sweep iterations on (X1, y1), a second upload, four more: as a fresh handle on (X2, y2) seeded with the
    state.  (L1: the second upload meets a w-step enqueued ahead of time.)"""
    d = WIDTH[storage]
    X1, y1 = _problem(N, d, 11)
    X2, y2 = _problem(N, d, 12)
    kw = dict(loss=loss, reg=0.01, wstep=getattr(R._lib, "WSTEP_" + wstep), storage=storage, tol=0.0)
    a = _fresh(R, X1, y1, d, kw)
    before = _steps(a, 4)
    assert before[-1][0] == 1 and before[-1][1] == 0, before[-1][:3]      # a look-ahead exists when the data are replaced
    a.set_data(X2, y2)
    a.gram()
    state = a.get_state()
    b = _fresh(R, X2, y2, d, kw)
    _seed(b, state)
    got, want = _steps(a, 4), _steps(b, 4)
    a.close()
    b.close()
    _assert_same(got, want)


# ------------------------------------------------------------------------------------------- 2. ... under a borrower
@pytest.mark.parametrize("wstep", ["L1", "L2"])
@pytest.mark.parametrize("storage,n,d", [("f32", N, WIDTH["f32"]), ("csr", 4096, 8)])
def test_owner_uploads_while_a_borrower_iterates(R, storage, n, d, wstep):
    """the owner uploads (X2, y2) and forms G again under a borrower that has iterated: the borrower goes on, without a
    set_state, as a fresh handle on (X2, y2) seeded with the borrower's state does, and holds the owner's new L"""
    X1, y1 = _problem(n, d, 21)
    X2, y2 = _problem(n, d, 22)
    if storage == "csr":
        sp = pytest.importorskip("scipy.sparse")
        rng = np.random.default_rng(5)
        X1, X2 = (sp.csr_matrix(X * (rng.random(X.shape) < 0.5)) for X in (X1, X2))
    kw = dict(loss=BCE, reg=0.01, wstep=getattr(R._lib, "WSTEP_" + wstep), storage=storage, tol=0.0)
    owner = _fresh(R, X1, y1, d, kw)
    b = R.Solver(n, d, "erm", share=owner, **kw)
    before = _steps(b, 3)
    assert before[-1][0] == (1 if storage == "f32" else 0) and before[-1][1] == 0, before[-1][:3]
    l_old = owner.info()["lipschitz"]
    owner.set_data(X2, y2)
    owner.gram()
    assert owner.info()["lipschitz"] != l_old
    twin = _fresh(R, X2, y2, d, kw)
    _seed(twin, b.get_state())
    got = _steps(b, 3)
    l_b, l_o = b.info()["lipschitz"], owner.info()["lipschitz"]
    want = _steps(twin, 3)
    for s in (b, twin, owner):
        s.close()
    assert l_b == l_o
    _assert_same(got, want)


# ----------------------------------------------------------------------------------- 3. finalize_smooth, then continue
def test_finalize_smooth_then_continue(R):
    d = WIDTH["f32"]
    X, y = _problem(N, d, 31)
    kw = dict(loss=BCE, reg=0.01, wstep=R._lib.WSTEP_SMOOTH_L1, storage="f32", tol=0.0)
    a = _fresh(R, X, y, d, kw)
    before = _steps(a, 4)
    assert before[-1][0] == 1 and before[-1][1] == 0, before[-1][:3]
    w_before = a.get_state()["w"]
    a.finalize_smooth()
    state = a.get_state()
    assert np.any(state["w"] != w_before)                 # the soft threshold moved w: the look-ahead belongs to another w
    b = _fresh(R, X, y, d, kw)
    _seed(b, state)
    got, want = _steps(a, 3), _steps(b, 3)
    a.close()
    b.close()
    _assert_same(got, want)
