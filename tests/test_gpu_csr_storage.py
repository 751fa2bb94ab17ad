"""Sparse storage of D on the device: include/rbl.h RBL_STORE_CSR, ``storage="csr"``.

D = -y X lives as its non-zero entries (row form for v = D w, column form for q = D^T c, float64 values), so the device
solves exactly the problem on ``toarray()``: every comparison below hands NumPy / the oracle the dense expansion and uses
the bars the dense tests use for the same check (tests/test_gpu_kernels.py, test_gpu_f16.py, test_gpu_group.py).

The designed 4099 x 1001 matrix comes in two forms, because one matrix cannot hold both empty rows and a column of 4099
entries (nor an empty column and a row of 1001): form "gaps" has the empty rows (first, last, a run), the rows with one
entry at column 0 and at column 1000, the empty column, a row over every other column and a column over every ordinary
row; form "full" has the row of 1001 and the column of 4099 entries.  Both hold the rows of 3 .. 257 entries, the columns
of 2^k - 1, 2^k, 2^k + 1 entries (k = 6 .. 11: every admissible segment length is crossed), explicit zeros and -0.0."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")
ST = "csr"


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _csr_from_mask(M, rng, zeros=True):
    """canonical CSR over the True cells of M: N(0, 1) values, explicit +0.0 / -0.0 among them"""
    rows, cols = np.nonzero(M)                       # row-major: canonical
    data = rng.standard_normal(rows.size)
    if zeros:
        data[3::37] = 0.0
        data[5::41] = -0.0
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M.shape[0]))]).astype(np.int32)
    A = sp.csr_matrix((data, cols.astype(np.int32), indptr), shape=M.shape)
    assert A.has_canonical_format and A.nnz == rows.size
    return A


ROW_LENGTHS = (3, 4, 5, 63, 64, 65, 128, 257)
COL_LENGTHS = tuple(2 ** k + e for k in range(6, 12) for e in (-1, 0, 1))


def _designed(form):
    n, d = 4099, 1001
    rng = np.random.default_rng(20 if form == "gaps" else 21)
    M = np.zeros((n, d), dtype=bool)
    special = list(range(0, 12)) + list(range(100, 105)) + [n - 1]
    ordinary = np.setdiff1d(np.arange(n), special)
    free = np.arange(40, 1000)                       # columns of the random fill
    M[np.ix_(ordinary, free)] = rng.random((ordinary.size, free.size)) < 0.01
    for j, length in enumerate(COL_LENGTHS):         # columns 10 .. 27: prescribed lengths
        M[rng.choice(ordinary, size=length - 1, replace=False), 10 + j] = True
    M[11, :] = True                                  # the long row (adds one entry to each column above)
    for i, length in enumerate(ROW_LENGTHS):         # rows 3 .. 10: prescribed lengths
        M[3 + i, rng.choice(free, size=length if form == "gaps" else length - 1, replace=False)] = True
    if form == "gaps":
        M[1, 0] = M[2, 1000] = True                  # single entries at the first and the last column
        M[ordinary, 5] = True                        # a column over every ordinary row
        M[:, 7] = False                              # the empty column
    else:
        M[:, 5] = True                               # the column of 4099 entries
        M[1, 0] = M[2, 1000] = True
    A = _csr_from_mask(M, rng)
    rl, cl = np.diff(A.indptr), np.bincount(A.indices, minlength=d)
    assert set(COL_LENGTHS) <= set(cl.tolist()) and set(ROW_LENGTHS) <= set(rl.tolist())
    if form == "gaps":
        assert rl[0] == rl[n - 1] == 0 and not rl[100:105].any() and rl[1] == rl[2] == 1 and rl[11] == d - 1
        assert A.indices[A.indptr[1]] == 0 and A.indices[A.indptr[2]] == 1000 and cl[7] == 0 and cl[5] == ordinary.size + 1
    else:
        assert rl[11] == d and cl[5] == n and rl.min() == 1
    assert (A.data == 0.0).sum() > 50 and np.signbit(A.data[A.data == 0.0]).any()
    return A


def _small(n, d, per_row, seed):
    rng = np.random.default_rng(seed)
    M = rng.random((n, d)) < per_row / d
    M[n // 2] = False
    return _csr_from_mask(M, rng)


@pytest.fixture(scope="module")
def cases():
    """name -> (A, dense D): the matrices of the parity and reproducibility tests, built once"""
    out = {"gaps": _designed("gaps"), "full": _designed("full"), "300x40": _small(300, 40, 5.0, 3), "257x4100": _small(257, 4100, 30.0, 4),
           # average rows of ~50, ~100, ~200 and ~300 entries: the lane groups of 8, 16, 32 and 64
           "150x2000": _small(150, 2000, 50.0, 6), "120x2000": _small(120, 2000, 100.0, 7), "110x2000": _small(110, 2000, 200.0, 8),
           "97x3000": _small(97, 3000, 300.0, 5)}
    for name, lo, hi in (("300x40", 0, 8), ("150x2000", 32, 64), ("120x2000", 64, 128), ("110x2000", 128, 256), ("97x3000", 256, 1e9)):
        assert lo < out[name].nnz / out[name].shape[0] <= hi, name
    assert out["300x40"].nnz / 300 < 8 and out["257x4100"].shape[1] > 4096
    return {k: (A, A.toarray()) for k, A in out.items()}


# ------------------------------------------------------------------------------------------------- 1. pass parity
@pytest.mark.parametrize("name", ["gaps", "full", "300x40", "257x4100", "150x2000", "120x2000", "110x2000", "97x3000"])
def test_pass_parity(R, cases, name):
    L = R._lib
    A, D = cases[name]
    n, d = D.shape
    ld = L.storage_ld(d, ST)
    rng = np.random.default_rng(9)
    w, c = rng.standard_normal(d), rng.standard_normal(n)
    v, q, G = L.k_csr_gemv(A, w), L.k_csr_gemvt(A, c), L.k_csr_gram(A)
    ev, eq, eg = np.max(np.abs(v - D @ w)), np.max(np.abs(q[:d] - D.T @ c)), np.max(np.abs(G - D.T @ D))
    bv, bq = 1e-13 * np.max(np.abs(D) @ np.abs(w) + 1), 1e-13 * np.max(np.abs(D.T) @ np.abs(c) + 1)
    print(f"csr {name}: |v - Dw| {ev:.2e} (bar {bv:.2e}), |q - DTc| {eq:.2e} (bar {bq:.2e}), |G - DTD| {eg:.2e} (bar {1e-12 * n:.2e})")
    assert ev <= bv and eq <= bq and eg <= 1e-12 * n
    assert q.shape == (ld,) and np.array_equal(_bits(q[d:]), np.zeros(ld - d, dtype=np.uint64))     # the padding: +0.0
    empty_rows, empty_cols = np.diff(A.indptr) == 0, np.bincount(A.indices, minlength=d) == 0
    assert np.array_equal(_bits(v[empty_rows]), np.zeros(empty_rows.sum(), dtype=np.uint64))
    assert np.array_equal(_bits(q[:d][empty_cols]), np.zeros(empty_cols.sum(), dtype=np.uint64))
    if name == "gaps":
        assert empty_rows.sum() == 7 and empty_cols.sum() >= 1
    assert np.array_equal(G, G.T)
    # the same pass run twice is bit-equal
    assert np.array_equal(_bits(L.k_csr_gemv(A, w)), _bits(v))
    assert np.array_equal(_bits(L.k_csr_gemvt(A, c)), _bits(q))
    assert np.array_equal(_bits(L.k_csr_gram(A)), _bits(G))


# --------------------------------------------------------------------------------------------- 2. reproducibility
def _dev(ptr, cnt):
    import torch
    from admm_for_rank_based_loss_amd.dist import _DevArray
    return torch.as_tensor(_DevArray(ptr, cnt), device="cuda:0").cpu().numpy().copy()


def _handle_vqG(R, src, y, w0, d):
    """v = D w0, q = D^T c of the first z-step and G, read from a superquantile handle that was given `src`"""
    L = R._lib
    n = y.size
    s = R.Solver(n, d, "superquantile", reg=0.01, wstep=L.WSTEP_L2, args=[0.5], storage=ST)
    s.set_data(src, y)
    s.gram()
    ld = s.info()["ld"]
    s.set_state(w=w0)
    s.phase_m()
    s.phase_z()
    s.phase_q()
    s.get_state()                                   # waits for the handle's stream
    out = (_dev(*s.buffer(L.BUF_V)), _dev(*s.buffer(L.BUF_Q))[:ld], _dev(*s.buffer(L.BUF_G)).reshape(ld, ld))
    s.close()
    return out


def test_sources_give_bit_equal_results(R, cases, monkeypatch):
    import torch
    A, D = cases["gaps"]
    n, d = D.shape
    rng = np.random.default_rng(12)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    w0 = 0.01 * rng.standard_normal(d)
    A32 = A.copy()
    A32.data = A.data.astype(np.float32).astype(np.float64)          # entries an f32 holds exactly
    Dy = -y[:, None] * A32.toarray()

    def variant(itype, vtype):
        B = sp.csr_matrix((A32.data.astype(vtype), A32.indices.astype(itype), A32.indptr.astype(itype)), shape=A32.shape)
        B.indices, B.indptr = B.indices.astype(itype), B.indptr.astype(itype)
        return B

    base = _handle_vqG(R, variant(np.int32, np.float64), y, w0, d)
    assert np.max(np.abs(base[0] - Dy @ w0)) <= 1e-13 * np.max(np.abs(Dy) @ np.abs(w0) + 1)
    assert np.max(np.abs(base[2][:d, :d] - Dy.T @ Dy)) <= 1e-12 * n
    assert np.any(base[1] != 0.0)
    runs = {"again": _handle_vqG(R, variant(np.int32, np.float64), y, w0, d),
            "int64": _handle_vqG(R, variant(np.int64, np.float64), y, w0, d),
            "f32": _handle_vqG(R, variant(np.int32, np.float32), y, w0, d),
            "int64 f32": _handle_vqG(R, variant(np.int64, np.float32), y, w0, d)}
    B = variant(np.int64, np.float64)
    t = torch.sparse_csr_tensor(torch.from_numpy(B.indptr), torch.from_numpy(B.indices), torch.from_numpy(B.data), size=B.shape).cuda()
    runs["device"] = _handle_vqG(R, t, y, w0, d)
    # five chunks of the host source: the planner's rule (csr_chunk_rows on the average row's share of the three arrays:
    # an int32 indptr entry plus 4 + 8 bytes per entry), restated
    per_row = 4 + (4 + 8) * -(-A32.nnz // n)
    cb = per_row * -(-n // 5)
    chunk = max(1, min(n, cb // per_row))
    assert -(-n // chunk) == 5
    monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", str(cb))
    runs["five chunks"] = _handle_vqG(R, variant(np.int32, np.float64), y, w0, d)
    monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES")
    for name, got in runs.items():
        for what, a, b in zip("vqG", got, base):
            assert np.array_equal(_bits(a), _bits(b)), (name, what, np.max(np.abs(a - b)))


# ------------------------------------------------------------------------------------------------------ 3. get_D
@pytest.mark.parametrize("ones", [False, True])
def test_get_D(R, cases, ones):
    import scaling_ref
    A, D = cases["gaps"]
    n, ds = D.shape
    y = np.where(np.random.default_rng(2).random(n) < 0.5, 1.0, -1.0)
    s = R.Solver(n, ds + (1 if ones else 0), "erm", reg=0.01, storage=ST, objective_only=True)
    s.set_data(A, y, ones_column=ones)
    got = s.get_D()
    want = scaling_ref.form_D(D, y, None, None, "f64", ones_column=ones)
    assert got.shape == want.shape and np.array_equal(got, want)         # values: -y * 0 is -+0.0 there, +0.0 here
    if ones:
        assert np.array_equal(got[:, -1], -y)
    assert not np.signbit(got[:, :ds][~_stored(A)]).any()                 # implicit entries: +0.0
    s.close()


def _stored(A):
    M = np.zeros(A.shape, dtype=bool)
    M[np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.indices] = True
    return M


# --------------------------------------------------------------------------------------------------- 4. refusals
def _set_csr(R, s, indptr, indices, data, y, nnz=None, scaling="none", flags=0):
    L = R._lib
    it = L.INDEX_DTYPE[indptr.dtype]
    return s.lib.rbl_set_data_csr(s._h, L.ptr(indptr), L.ptr(indices), L.ptr(data), int(data.size if nnz is None else nnz), it,
                                  L.SOURCE_DTYPE[data.dtype], L.MEM_HOST, L.ptr(y), L.SCALING[scaling], flags)


def test_refusals_leave_the_handle_without_data(R, cases):
    L = R._lib
    A, D = cases["300x40"]
    n, d = D.shape
    y = np.where(np.random.default_rng(6).random(n) < 0.5, 1.0, -1.0)
    Dy = -y[:, None] * D
    s = R.Solver(n, d, "erm", reg=0.01, wstep=L.WSTEP_L1, storage=ST)
    r = int(np.argmax(np.diff(A.indptr) >= 3))
    a = A.indptr[r]

    def after(msg):
        """the refusal's message; the handle has no data; a valid upload then works"""
        with pytest.raises(ValueError, match=msg):
            L.check(code)
        with pytest.raises(Exception, match="set_data|no data"):
            s.step(False)
        with pytest.raises(Exception, match="no data"):
            s.get_D()
        s.set_data(A, y)
        assert np.array_equal(s.get_D(), Dy)

    s.set_data(A, y)
    bad = A.indices.copy()
    bad[a + 1] = d
    code = _set_csr(R, s, A.indptr, bad, A.data, y)
    after(rf"set_data_csr: \d+ entries refused, first in row {r}: column index {d} \(entry 1 of the row\) is outside \[0, {d}\)")
    bad = A.indices.copy()
    bad[a + 1] = bad[a]
    code = _set_csr(R, s, A.indptr, bad, A.data, y)
    after(rf"first in row {r}: column index {bad[a]} is repeated \(entries 0 and 1 of the row\)")
    bad = A.indices.copy()
    bad[a + 1], bad[a + 2] = A.indices[a + 2], A.indices[a + 1]
    code = _set_csr(R, s, A.indptr, bad, A.data, y)
    after(rf"first in row {r}: column index {bad[a + 2]} follows {bad[a + 1]} .* must be strictly increasing")
    for scaling in ("fit", "apply"):
        code = _set_csr(R, s, A.indptr, A.indices, A.data, y, scaling=scaling)
        assert code == L.RBL_ERR_INVALID
        after("RBL_SCALE_FIT / RBL_SCALE_APPLY on a handle with RBL_STORE_CSR - centring")
    code = s.lib.rbl_set_data_from(s._h, L.ptr(D), L.DTYPE_F64, L.MEM_HOST, d, L.ptr(y), 0, 0)
    assert code == L.RBL_ERR_INVALID
    after("set_data_from: a dense source on a handle with RBL_STORE_CSR")
    code = s.lib.rbl_set_data(s._h, L.ptr(D), L.ptr(y), d)
    after("a dense source on a handle with RBL_STORE_CSR")
    code = s.lib.rbl_generate_synthetic(s._h, 7, 1.0, 0.01)
    assert code == L.RBL_ERR_INVALID
    after("generate_synthetic: the synthetic generator writes a dense matrix")
    code = s.lib.rbl_synth_local(s._h, 7, 1.0, 0.01)
    after("synth_local: the synthetic generator writes a dense matrix")
    code = s.lib.rbl_set_data_csr(s._h, L.ptr(A.indptr), None, None, 2 ** 31, L.INDEX_I32, L.DTYPE_F64, L.MEM_HOST, L.ptr(y), 0, 0)
    assert code == L.RBL_ERR_INVALID
    after(r"nnz = 2147483648 exceeds the 2\^31 - 1 entries")
    code = s.lib.rbl_set_data_csr(s._h, L.ptr(A.indptr), None, None, 2 ** 31 - n, L.INDEX_I32, L.DTYPE_F64, L.MEM_HOST, L.ptr(y), 0,
                                  L.DATA_ONES_COLUMN)
    after(r"nnz = \d+ \(plus n for the column of ones\) exceeds")
    s.close()
    with pytest.raises(ValueError, match=r"RBL_STORE_CSR: row-sharded handles \(n = 100 of n_total = 300\)"):
        R.Solver(100, d, "erm", reg=0.01, storage=ST, n_total=300, row_offset=0)
    # the Python layer says it first
    s = R.Solver(n, d, "erm", reg=0.01, storage=ST, objective_only=True)
    with pytest.raises(ValueError, match=r"scipy\.sparse\.csr_matrix\(X\)"):
        s.set_data(D, y)
    with pytest.raises(ValueError, match='standardize=True with storage="csr"'):
        s.set_data(A, y, scaling="fit")
    s.close()


# ------------------------------------------------------------------------- 5. iterates against the oracle's exact mode
FAM = {
    "erm_l1": dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01),
    "superq": dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5]),
    "aorr_hinge": dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
    "ehrm": dict(weight_function="ehrm", loss="binary_cross_entropy", l2_reg=0.01, B=-5),
    "extremile_l1": dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
    "superq_sqhinge": dict(weight_function="superquantile", loss="squared_hinge", l2_reg=0.01, args=[0.5]),
}
SHAPES = [(2000, 60, False), (1501, 300, True)]


def _sparse_problem(n, d, intercept, density=0.15):
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=700 + n + d, intercept=intercept)
    keep = np.random.default_rng(n + d).random(X.shape) < density
    if intercept:
        keep[:, -1] = True
    X = X * keep
    A = sp.csr_matrix(X)
    return A, A.toarray(), y


_REF = {}


def _oracle(fam, n, d, intercept, nit):
    """the oracle's exact-mode run on toarray(), computed once per case and shared"""
    from oracle import admm
    key = (fam, n, d, intercept, nit)
    if key not in _REF:
        A, X, y = _sparse_problem(n, d, intercept)
        kw = FAM[fam]
        if kw["loss"] == "squared_hinge":           # the NumPy restatement of the oracle's exact mode for this loss
            import sqhinge_ref
            ref = sqhinge_ref.admm(X, y, max_iter=nit, tol=0.0, **{k: v for k, v in kw.items() if k != "loss"})
        else:
            ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw)
        _REF[key] = (A, X, y, ref)
    return _REF[key]


def _run(R, X, y, kw, nit, storage):
    s = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=storage, **kw)._s
    hist = []
    for _ in range(nit):
        st = s.step(True)
        hist.append((st.primal, st.dual, st.rho, st.objective, st.ehrm_branch, st.fused, st.fused_v))
    state = s.get_state()
    s.close()
    return np.array(hist), state


@pytest.mark.parametrize("n,d,intercept", SHAPES, ids=[f"{n}x{d + (1 if i else 0)}" for n, d, i in SHAPES])
@pytest.mark.parametrize("fam", list(FAM))
def test_iterates_against_the_oracle(R, fam, n, d, intercept):
    kw, nit = FAM[fam], 8
    A, X, y, ref = _oracle(fam, n, d, intercept, nit)
    tol = 1e-7 if kw["loss"] == "hinge" else 1e-9        # hinge: the kinks amplify rounding
    h, st = _run(R, A, y, kw, nit, ST)
    assert not h[:, 5].any() and not h[:, 6].any()       # fused == 0 and fused_v == 0 in every step
    assert np.allclose(h[:, 2], ref.rho, rtol=1e-15)
    assert np.allclose(h[:, 0], ref.primal, rtol=tol, atol=tol), (h[:, 0], ref.primal)
    assert np.allclose(h[:, 1], ref.dual, rtol=tol, atol=tol)
    assert np.allclose(h[:, 3], ref.objective[1:], rtol=tol, atol=tol)
    if fam == "ehrm":
        assert [int(b) for b in h[:, 4]] == [0 if b == "a" else 1 for b in ref.branch]
    assert np.max(np.abs(st["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w)))
    assert np.max(np.abs(st["z"] - ref.z)) <= 10 * tol * max(1.0, np.max(np.abs(ref.z)))
    assert np.max(np.abs(st["lam"] - ref.lam)) <= 10 * tol * max(1e-3, np.max(np.abs(ref.lam)))


# ------------------------------------------------------------------------- 6. the same solve with dense and sparse D
@pytest.mark.parametrize("fam", ["erm_l1", "superq", "ehrm", "extremile_l1"])
def test_dense_and_sparse_storage_agree(R, fam):
    n, d, intercept = SHAPES[0]
    A, X, y = _sparse_problem(n, d, intercept)
    nit, tol = 8, 1e-9
    hd, sd = _run(R, A, y, FAM[fam], nit, "f64")
    hs, ss = _run(R, A, y, FAM[fam], nit, ST)
    assert np.allclose(hs[:, 2], hd[:, 2], rtol=1e-15)
    for col in (0, 1, 3):
        assert np.allclose(hs[:, col], hd[:, col], rtol=tol, atol=tol), col
    assert np.array_equal(hs[:, 4], hd[:, 4])
    assert np.max(np.abs(ss["w"] - sd["w"])) <= tol * max(1.0, np.max(np.abs(sd["w"])))
    assert np.max(np.abs(ss["z"] - sd["z"])) <= 10 * tol * max(1.0, np.max(np.abs(sd["z"])))
    assert np.max(np.abs(ss["lam"] - sd["lam"])) <= 10 * tol * max(1e-3, np.max(np.abs(sd["lam"])))


# ------------------------------------------------------------------------------------------------ 7. Python surface
def test_admmmethod_with_a_sparse_test_set(R):
    from oracle import admm
    A, X, y = _sparse_problem(1200, 50, False)
    At, Xt, yt = _sparse_problem(500, 50, False, density=0.2)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    s = R.ADMMmethod(A, y, max_iter=6, tol=0.0, storage=ST, fit_intercept=True, **kw)
    s.start_store(At, yt, kw["weight_function"], kw["loss"], l2_reg=0.01, args=[0.5])
    w = _quiet(s.main_loop)
    assert w.shape == (51, 1) and len(s.test_losses) == 7 and np.all(np.isfinite(s.test_losses))
    d = R.ADMMmethod(A, y, max_iter=6, tol=0.0, storage="f64", fit_intercept=True, **kw)
    d.start_store(Xt, yt, kw["weight_function"], kw["loss"], l2_reg=0.01, args=[0.5])
    wd = _quiet(d.main_loop)
    assert np.max(np.abs(w - wd)) <= 1e-9 * max(1.0, np.max(np.abs(wd)))
    assert np.allclose(s.test_losses, d.test_losses, rtol=1e-9, atol=1e-9)
    assert np.allclose(s.train_losses, d.train_losses, rtol=1e-9, atol=1e-9)


def test_group_of_three_levels_runs_the_members_own_passes(R):
    A, X, y = _sparse_problem(1500, 80, False)
    nit = 6
    problems = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[a]) for a in (0.5, 0.9, 0.3)]
    g = R.ADMMgroup(A, y, problems, storage=ST, max_iter=nit, tol=0.0)
    ws = _quiet(g.main_loop, verbose=False)
    cnt = g.counters()
    assert cnt["k_per_pass"] == 1 and cnt["shared_v"] == 0 and cnt["shared_q"] == 0, cnt
    assert all(c >= 2 * nit for c in cnt["single_passes"]), cnt
    for pr, w in zip(problems, ws):
        a = R.ADMMmethod(A, y, max_iter=nit, tol=0.0, storage=ST, **pr)
        wa = _quiet(a.main_loop, verbose=False)
        assert np.max(np.abs(w - wa)) <= 1e-11 * max(1.0, np.max(np.abs(wa)))
        f = R.ADMMmethod(A, y, max_iter=nit, tol=0.0, storage="f64", **pr)
        wf = _quiet(f.main_loop, verbose=False)
        assert np.max(np.abs(w - wf)) <= 1e-9 * max(1.0, np.max(np.abs(wf)))
    g.close()


def _blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((3, d)) / np.sqrt(d)
    labels = rng.integers(0, 3, size=n)
    X = (rng.standard_normal((n, d)) + centres[labels]) * (rng.random((n, d)) < 0.3)
    return sp.csr_matrix(X), np.array(["a", "b", "c"])[labels]


def test_one_vs_rest(R):
    n, d, nit = 1500, 120, 10
    A, lab = _blobs(n, d, seed=2)
    At, _ = _blobs(600, d, seed=2)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    ovr = R.OneVsRest(A, lab, storage=ST, max_iter=nit, tol=0.0, **kw)
    W = _quiet(ovr.main_loop, verbose=False)
    cnt = ovr.group.counters()
    assert cnt["k_per_pass"] == 1 and cnt["shared_v"] == cnt["shared_q"] == 0, cnt
    pred = ovr.predict(At)
    dense = R.OneVsRest(A, lab, storage="f64", max_iter=nit, tol=0.0, **kw)
    Wd = _quiet(dense.main_loop, verbose=False)
    pd_ = dense.predict(At)
    assert np.max(np.abs(W - Wd)) <= 1e-9 * max(1.0, np.max(np.abs(Wd)))
    Xt = At.toarray()
    sc = Xt @ Wd
    top = np.sort(sc, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(Xt) @ np.abs(Wd) + 1, axis=1)
    assert keep.sum() >= 0.99 * len(keep)
    assert np.array_equal(pred[keep], pd_[keep])
    assert np.array_equal(pred[keep], ovr.classes_[np.argmax(sc, axis=1)][keep])
    ovr.close()
    dense.close()


def test_relabelled_borrower_equals_a_handle_of_its_own(R):
    A, X, y = _sparse_problem(1500, 80, False)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    yk = np.where(np.random.default_rng(4).random(y.size) < 0.4, 1.0, -1.0)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    nit = 6
    owner = R.ADMMmethod(A, y, max_iter=nit, tol=0.0, storage=ST, **kw)
    b = R.ADMMmethod(A, yk, max_iter=nit, tol=0.0, storage=ST, share_data=owner, **kw)
    own = R.ADMMmethod(A, yk, max_iter=nit, tol=0.0, storage=ST, **kw)
    assert np.array_equal(b._s.get_D(), -yk[:, None] * X)
    for _ in range(nit):
        b._s.step(False)
        own._s.step(False)
    sb, so = b._s.get_state(), own._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(_bits(sb[key]), _bits(so[key])), (key, np.max(np.abs(sb[key] - so[key])))
    assert sb["rho"] == so["rho"]


def test_second_upload_under_a_borrower_after_a_refused_call(R):
    """owner + borrower at ld = 8, a refused call on the owner, then a second upload with so many more entries that the
    segments of q = D^T c outnumber the doubles of the slab the borrower was created with: the borrower's slab follows
    (its pass would otherwise write past it), and the borrower matches a handle of its own on the new data"""
    L = R._lib
    n, d = 4_400_000, 8
    rng = np.random.default_rng(31)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    one = sp.csr_matrix((rng.standard_normal(n), rng.integers(0, d, size=n).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, d))
    full = sp.csr_matrix((rng.standard_normal(n * d), np.tile(np.arange(d, dtype=np.int32), n), np.arange(n + 1, dtype=np.int64) * d),
                         shape=(n, d))
    kw = dict(reg=0.01, wstep=L.WSTEP_L2, storage=ST, tol=0.0)
    owner = R.Solver(n, d, "erm", **kw)
    owner.set_data(one, y)
    owner.gram()
    b = R.Solver(n, d, "erm", share=owner, **kw)
    slab_doubles = owner.info()["num_cu"] * 4 * owner.info()["ld"] * 2       # gemvt_slab_rows(num_cu) x ld x 2: a borrower's slab
    assert -(-one.nnz // d // 2048) * d + d < slab_doubles < (n // 2048) * d, slab_doubles
    b.step(False)
    with pytest.raises(ValueError, match="RBL_SCALE_FIT / RBL_SCALE_APPLY on a handle with RBL_STORE_CSR"):
        L.check(_set_csr(R, owner, one.indptr, one.indices, one.data, y, scaling="fit"))
    b.step(False)                                    # the borrower still runs on the data that stand
    owner.set_data(full, y)                          # regrows the buffers under the borrower
    owner.gram()
    own = R.Solver(n, d, "erm", **kw)
    own.set_data(full, y)
    own.gram()
    w0 = 0.01 * rng.standard_normal(d)
    for s in (b, own):
        s.set_state(w=w0, z=np.zeros(n), lam=np.zeros(n), rho=1e-5, iter=0)
        for _ in range(2):
            st = s.step(True)
        assert np.isfinite(st.objective) and st.fused == 0
    sb, so = b.get_state(), own.get_state()
    for key in ("w", "z", "lam"):       # tests/test_gpu_group.py's bar for "the same maths" on two handles
        assert np.max(np.abs(sb[key] - so[key])) <= 1e-11 * max(1e-3 if key == "lam" else 1.0, np.max(np.abs(so[key]))), key
    assert np.any(sb["w"] != w0)
    # an upload that fails half way - with another entry count, so the entry buffers are new and unwritten where an entry
    # was refused - leaves the borrower with an error, not with entries to read: its passes and its get_D refuse
    bad = one.indices.copy()
    bad[5] = d
    with pytest.raises(ValueError, match="is outside"):
        L.check(_set_csr(R, owner, one.indptr, bad, one.data, y))
    with pytest.raises(L.RblError, match="data are not complete"):
        b.step(False)
    with pytest.raises(L.RblError, match="csr dense: the data are not complete"):
        b.get_D()
    with pytest.raises(L.RblError, match="data are not complete"):
        b.objective(w0)
    owner.set_data(one, y)
    owner.gram()
    b.set_state(w=w0, z=np.zeros(n), lam=np.zeros(n), rho=1e-5, iter=0)
    assert np.isfinite(b.step(True).objective)
    for s in (b, own, owner):
        s.close()


def test_dense_kernel_entries_refuse_the_sparse_storage_id(R):
    L = R._lib
    D = np.ones((4, 3))
    for call in (lambda: L.load().rbl_k_gemv(3, 4, 3, L.ptr(D), L.ptr(np.ones(3)), L.ptr(np.empty(4))),
                 lambda: L.load().rbl_k_gemvt(3, 4, 3, L.ptr(D), L.ptr(np.ones(4)), L.ptr(np.empty(3))),
                 lambda: L.load().rbl_k_gram(3, 4, 3, L.ptr(D), L.ptr(np.empty((3, 3)))),
                 lambda: L.load().rbl_k_gemv(7, 4, 3, L.ptr(D), L.ptr(np.ones(3)), L.ptr(np.empty(4)))):
        with pytest.raises(ValueError, match="storage must be RBL_STORE_F32, RBL_STORE_F64 or RBL_STORE_F16"):
            L.check(call())


# ------------------------------------------------------------------------------------------------------ 8. memory
def test_sparse_handle_takes_a_fraction_of_the_dense_memory(R):
    """an objective-only erm handle of 400 000 x 4096 with 20 entries per row, measured after set_data as
    tests/test_gpu_f16.py::test_fp16_handle_takes_little_more_than_half_the_memory measures: below a tenth of n ld 4 bytes
    (dense fp32: 6.5 GB; the entries take 8 M x 12 bytes = 96 MB in the row form an objective-only handle keeps, the
    n-vectors a few tens of MB)"""
    import torch
    n, d, per_row = 400_000, 4096, 20
    rng = np.random.default_rng(8)
    step = d // per_row
    indices = (np.arange(per_row, dtype=np.int32) * step)[None, :] + rng.integers(0, step, size=(n, per_row), dtype=np.int32)
    A = sp.csr_matrix((rng.standard_normal(n * per_row), indices.reshape(-1), np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, d))
    A.indices = A.indices.astype(np.int64)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    u0 = used()
    s = R.Solver(n, d, "erm", storage=ST, objective_only=True)
    s.set_data(A, y)
    took = used() - u0
    w = rng.standard_normal(d)
    acc = s.accuracy(w)
    s.close()
    print(f"400000 x 4096, 20 entries per row, objective-only csr handle: {took / 1e6:.1f} MB (dense f32: {n * d * 4 / 1e6:.0f} MB)")
    assert took < 0.1 * n * R._lib.storage_ld(d, ST) * 4, took
    assert 0.4 < acc < 0.6
