"""Scale-only standardisation on the device: include/rbl.h rbl_set_centering, ``standardize="scale"``.

With centring off RBL_SCALE_FIT / APPLY divide the columns by their population standard deviation and subtract nothing, so
a handle with RBL_STORE_CSR takes them and D stays sparse.  The vectors of the sparse FIT are compared in bits with the
NumPy restatement of the statistics kernels (tests/scale_only_ref.py); stored values, whole solves and test objectives with
the same quantities of a handle given the host-prescaled matrix - the two run identical kernels on identical bits."""
import contextlib
import io

import numpy as np
import pytest

import scale_only_ref as ref

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")


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


def _csr(X, M):
    """canonical CSR over the True cells of M, values from X (zeros stay as explicit entries)"""
    rows, cols = np.nonzero(M)
    indptr = np.concatenate([[0], np.cumsum(M.sum(axis=1))]).astype(np.int32)
    A = sp.csr_matrix((X[rows, cols], cols.astype(np.int32), indptr), shape=M.shape)
    assert A.has_canonical_format and A.nnz == rows.size
    return A


def _labels(n, seed):
    return np.where(np.random.default_rng(seed).random(n) < 0.5, 1.0, -1.0)


def _prescaled(A, scale):
    """csr(A . diag(1.0 / scale)) with A's structure: the multiplication the device does, on the host"""
    B = A.copy()
    B.data = A.data.astype(np.float64) * (1.0 / np.asarray(scale))[A.indices]
    return B


# ------------------------------------------------------------------------------- 1. the vectors of the sparse FIT
@pytest.fixture(scope="module")
def designed():
    """2500 x 40, values exact in float16 (so float64 / float32 / float16 sources hold the same numbers): a full column
    is 2500 entries - two segments of RBL_CSC_SEG = 2048"""
    n, d = 2500, 40
    rng = np.random.default_rng(31)
    X = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-1, 2, size=d)).astype(np.float16).astype(np.float64)
    M = rng.random((n, d)) < 0.05
    X[M & (rng.random((n, d)) < 0.03)] = 0.0             # explicit zeros among the ordinary columns
    M[:, 0] = True
    X[:, 0] = float(np.float16(0.7))                     # a full constant column
    M[:, 1] = True                                       # a full varying column
    X[:, 1] += 3.0
    X[:, 1] = X[:, 1].astype(np.float16)
    M[:, 2] = False                                      # an empty column
    M[:, 3] = False
    M[1234, 3] = True                                    # a single entry
    X[1234, 3] = 2.5
    M[:, 4] = rng.random(n) < 0.1                        # explicit zeros and -0.0 only
    X[:, 4] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    M[:, 5] = True                                       # 2100 entries, not full: the list straddles the segment boundary
    M[rng.choice(n, size=400, replace=False), 5] = False
    A = _csr(X, M)
    cl = np.bincount(A.indices, minlength=d)
    assert cl[0] == cl[1] == n and cl[2] == 0 and cl[3] == 1 and cl[5] == 2100 and 0 < cl[4] < n
    assert np.signbit(X[M[:, 4], 4]).any() and not X[M[:, 4], 4].any()
    y = _labels(n, 32)
    mean, scale = ref.fit_csr(A)
    assert scale[0] == scale[2] == scale[4] == 1.0 and (scale[[1, 3, 5]] != 1.0).all()
    return A, y, mean, scale


def _fit(R, src, y, n, d, ones=False):
    s = R._solver.Solver(n, d + (1 if ones else 0), "erm", reg=0.01, storage="csr")
    try:
        s.set_centering(False)
        assert s.get_centering() is False
        s.set_data(src, y, scaling="fit", ones_column=ones)
        mean, scale = s.get_scaling()
        stats_ms, launches = s.kernel_time(R._lib.KERNEL_SRC_STATS)      # the statistics launches of this upload
        assert launches == 1 and stats_ms > 0.0
        return mean, scale, s.get_D()
    finally:
        s.close()


def _typed_source(R, A, vt, it):
    S = R._solver
    L = R._lib
    indptr, indices = A.indptr.astype(it), A.indices.astype(it)
    data = A.data.astype(vt)
    assert np.array_equal(data.astype(np.float64), A.data)
    return S.CsrSource(A.shape, L.SOURCE_DTYPE[np.dtype(vt)], L.MEM_HOST, L.INDEX_DTYPE[np.dtype(it)], data.shape[0],
                       indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, (indptr, indices, data))


@pytest.mark.parametrize("variant", ["f64-i32", "f64-i64", "f32-i32", "f16-i64", "device", "chunks", "ones"])
def test_sparse_fit_vectors(R, designed, variant, monkeypatch):
    A, y, _, want = designed
    n, d = A.shape
    ones = variant == "ones"
    if variant == "device":
        import torch
        src = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                      torch.from_numpy(A.data), size=A.shape).to("cuda:0")
    elif variant in ("chunks", "ones"):
        if variant == "chunks":
            monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", "4096")       # a few hundred rows a chunk
        src = A
    else:
        vt, it = variant.split("-")
        src = _typed_source(R, A, {"f64": np.float64, "f32": np.float32, "f16": np.float16}[vt], {"i32": np.int32, "i64": np.int64}[it])
    mean, scale, D = _fit(R, src, y, n, d, ones)
    assert not mean.any() and not np.signbit(mean).any()
    assert np.array_equal(_bits(scale[:d]), _bits(want))
    if ones:
        assert scale[d] == 1.0 and np.array_equal(D[:, d], -y)
    # the stored values: fl((-y x) * fl(1 / scale)); explicit zeros and -0.0 keep their bits
    B = _prescaled(A, want)
    Dw = -y[:, None] * B.toarray()
    assert np.array_equal(D[:, :d], Dw)
    r, c = np.repeat(np.arange(n), np.diff(A.indptr)), A.indices
    assert np.array_equal(_bits(D[r, c]), _bits(-y[r] * B.data))


# --------------------------------------------------------------------------------- 2. APPLY, a prescribed vector
@pytest.mark.parametrize("objective_only", [True, False])
@pytest.mark.parametrize("ones", [False, True])
def test_apply_matches_dense_and_numpy(R, designed, objective_only, ones):
    A, y, _, _ = designed
    n, d = A.shape
    rng = np.random.default_rng(7)
    scale = np.exp(rng.standard_normal(d))               # not the fitted ones: any positive vector
    zeros = np.zeros(d)
    got = {}
    for storage, src in (("csr", A), ("f64", A.toarray())):
        s = R._solver.Solver(n, d + (1 if ones else 0), "erm", reg=0.01, storage=storage, objective_only=objective_only)
        s.set_centering(False)
        s.set_scaling(*R._solver.as_scaling(zeros, scale, s.d, ones))
        s.set_data(src, y, scaling="apply", ones_column=ones)
        m2, s2 = s.get_scaling()
        assert not m2.any() and np.array_equal(s2[:d], scale)
        got[storage] = s.get_D()
        s.close()
    want = -y[:, None] * (A.toarray() * (1.0 / scale))
    if ones:
        want = np.hstack([want, -y[:, None]])
    assert np.array_equal(got["csr"], want) and np.array_equal(got["f64"], want)
    r, c = np.repeat(np.arange(n), np.diff(A.indptr)), A.indices
    # stored entries: the sign of an explicit -0.0 too (toarray() adds it to +0.0 and loses it: taken from A.data)
    assert np.array_equal(_bits(got["csr"][r, c]), _bits(-y[r] * (A.data * (1.0 / scale)[c])))
    assert np.array_equal(_bits(got["f64"]), _bits(want))


# ------------------------------------------------------------------------------ 3. dense storage, centring off
@pytest.mark.parametrize("storage", ["f32", "fp16"])
@pytest.mark.parametrize("ones", [False, True])
def test_dense_fit_without_centring(R, storage, ones):
    n, d = 1500, 37
    rng = np.random.default_rng(41)
    X = (rng.standard_normal((n, d)) * np.exp(rng.standard_normal(d)) + rng.standard_normal(d) * 3.0).astype(np.float32)
    X[:, 5] = 1.25                                       # a constant column: scale 1
    y = _labels(n, 42)
    out = {}
    for center in (True, False):
        s = R._solver.Solver(n, d + (1 if ones else 0), "erm", reg=0.01, storage=storage, objective_only=True)
        s.set_centering(center)
        s.set_data(X, y, scaling="fit", ones_column=ones)
        out[center] = s.get_scaling() + (s.get_D(),)
        s.close()
    mean, scale, D = out[False]
    assert np.array_equal(_bits(scale), _bits(out[True][1])) and scale[5] == 1.0
    assert not mean.any() and out[True][0][:d].any()
    want = -y[:, None] * (X.astype(np.float64) * (1.0 / scale[:d]))
    if ones:
        want = np.hstack([want, -y[:, None]])
    want = R._lib.storage_round(want, storage)
    assert np.array_equal(_bits(D), _bits(want))


# ------------------------------------------------------------------------------------ 4. whole solves, bit for bit
def _random_csr(n, d, per_row, seed):
    rng = np.random.default_rng(seed)
    M = rng.random((n, d)) < per_row / d
    X = rng.standard_normal((n, d)) * np.exp(rng.standard_normal(d)) + 0.5
    return _csr(X, M)


@pytest.mark.parametrize("case", ["erm-l1", "superquantile-l2", "wide-operator", "wide-working-set"])
def test_solves_match_the_prescaled_matrix(R, case):
    kw = dict(storage="csr", fit_intercept=True, max_iter=12, tol=1e-12)
    if case == "erm-l1":
        A, kw2 = _random_csr(400, 30, 6.0, 51), dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01)
    elif case == "superquantile-l2":
        A, kw2 = _random_csr(400, 30, 6.0, 52), dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.05, args=[0.5])
    else:
        A = _random_csr(60, 20000, 5.0, 53)
        kw2 = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, gram="auto")
        if case == "wide-working-set":
            kw2["l1_solver"] = "working_set"
    y = _labels(A.shape[0], 54)
    a = R.ADMMmethod(A, y, standardize="scale", **kw, **kw2)
    assert not a.scale_mean_.any() and a.scale_scale_.shape == (A.shape[1],)
    if case.startswith("wide"):
        assert a.gram == "none"
    b = R.ADMMmethod(_prescaled(A, a.scale_scale_), y, **kw, **kw2)
    wa, wb = _quiet(a.main_loop, verbose=False), _quiet(b.main_loop, verbose=False)
    assert np.abs(wa).max() > 0 and np.array_equal(_bits(wa), _bits(wb))
    coef, icpt = a.unscaled()
    assert np.array_equal(_bits(coef), _bits(a.coef_ / a.scale_scale_)) and icpt == a.intercept_


def test_one_vs_rest_matches_the_prescaled_matrix(R):
    A = _random_csr(450, 24, 6.0, 55)
    labels = np.random.default_rng(56).integers(0, 3, size=A.shape[0])
    kw = dict(l2_reg=0.05, storage="csr", fit_intercept=True, share_sparse=True, max_iter=10, tol=1e-12)
    a = R.OneVsRest(A, labels, standardize="scale", **kw)
    b = R.OneVsRest(_prescaled(A, a.scale_scale_), labels, **kw)
    Wa, Wb = _quiet(a.main_loop, verbose=False), _quiet(b.main_loop, verbose=False)
    assert np.abs(Wa).max() > 0 and np.array_equal(_bits(Wa), _bits(Wb))
    At = _random_csr(200, 24, 6.0, 57)
    assert np.array_equal(a.predict(At), b.predict(_prescaled(At, a.scale_scale_)))
    a.close()
    b.close()


# --------------------------------------------------------------------- 5. the model of full standardisation
@pytest.mark.parametrize("loss", ["binary_cross_entropy", "hinge"])
def test_objective_equals_full_standardisation(R, loss):
    """rbl_objective (erm: the mean loss) of the dense f64 centred-APPLY handle at (w, b) against the csr scale-only handle
    at (w, b - sum_j w_j mean_j / scale_j).  Both losses are 1-Lipschitz in the margin, so the two values differ by at
    most the largest difference of two margins: (d + 3) 2^-52 max_i sum_j |w_j| (|x_ij| + |mean_j|) / scale_j."""
    n, d = 300, 12
    rng = np.random.default_rng(61)
    M = rng.random((n, d)) < 0.4
    X = np.where(M, rng.standard_normal((n, d)) * np.exp(rng.standard_normal(d)) + rng.standard_normal(d), 0.0)
    A = _csr(X, M)
    y = _labels(n, 62)
    mean, scale = ref.fit_csr(A)
    full = R._solver.Solver(n, d + 1, "erm", loss, storage="f64", objective_only=True)
    full.set_scaling(*R._solver.as_scaling(mean, scale, d + 1, True))
    full.set_data(X, y, scaling="apply", ones_column=True)
    only = R._solver.Solver(n, d + 1, "erm", loss, storage="csr", objective_only=True)
    only.set_centering(False)
    only.set_scaling(*R._solver.as_scaling(np.zeros(d), scale, d + 1, True))
    only.set_data(A, y, scaling="apply", ones_column=True)
    for trial in range(5):
        w, b = rng.standard_normal(d), float(rng.standard_normal())
        w2, b2 = ref.map_point(w, b, mean, scale)
        f1, f2 = full.risk(np.append(w, b)), only.risk(np.append(w2, b2))
        bound = (d + 3) * 2.0 ** -52 * float(np.max((np.abs(X) + np.abs(mean)) / scale @ np.abs(w)))
        print(f"{loss} trial {trial}: {f1:.17g} {f2:.17g} difference {abs(f1 - f2):.3e} bound {bound:.3e}")
        assert f1 > 0 and abs(f1 - f2) <= bound
    full.close()
    only.close()


# ------------------------------------------------------------------------------- 6. start_store, a sparse test set
def test_start_store_on_a_sparse_test_matrix(R):
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
    A, At = _random_csr(400, 30, 6.0, 71), _random_csr(250, 30, 6.0, 72)
    y, yt = _labels(400, 73), _labels(250, 74)
    w0 = np.random.default_rng(75).standard_normal(31) * 0.3
    kw = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, storage="csr", fit_intercept=True, max_iter=8,
              tol=1e-12, w0=w0)
    a = R.ADMMmethod(A, y, standardize="scale", **kw)
    scale = a.scale_scale_
    b = R.ADMMmethod(_prescaled(A, scale), y, **kw)
    a.start_store(At, yt, l1_reg=0.01)
    b.start_store(_prescaled(At, scale), yt, l1_reg=0.01)
    _quiet(a.main_loop, verbose=False)
    _quiet(b.main_loop, verbose=False)
    assert len(a.test_losses) > 1 and a.test_losses[0] != a.test_losses[-1]
    assert a.test_losses == b.test_losses and a.train_losses == b.train_losses
    w = a.w.reshape(-1)
    acc = calculate_accuracy(w, At, yt, scaling=(a.scale_mean_, a.scale_scale_), storage="csr")
    ones = sp.csr_matrix(np.ones((250, 1)))
    assert acc == calculate_accuracy(w, sp.hstack([_prescaled(At, scale), ones]).tocsr(), yt, storage="csr")
    assert 0.0 < acc < 1.0


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_their_reason_and_leave_the_handle_usable(R, designed):
    L = R._lib
    A, y, _, want = designed
    n, d = A.shape
    s = R._solver.Solver(n, d, "erm", reg=0.01, storage="csr")

    def fit_code():
        return s.lib.rbl_set_data_csr(s._h, L.ptr(A.indptr), L.ptr(A.indices), L.ptr(A.data), A.nnz, L.INDEX_DTYPE[A.indptr.dtype],
                                      L.SOURCE_DTYPE[A.data.dtype], L.MEM_HOST, L.ptr(y), L.SCALING["fit"], 0)

    assert s.get_centering() is True
    assert fit_code() == L.RBL_ERR_INVALID                # csr + FIT with centring on: the old message
    assert "RBL_SCALE_FIT / RBL_SCALE_APPLY on a handle with RBL_STORE_CSR - centring the columns makes D dense" in L.last_error()
    s.set_centering(False)
    assert fit_code() == L.RBL_OK
    assert np.array_equal(_bits(s.get_scaling()[1]), _bits(want))
    # APPLY with a mean that is not all zeros
    mean = np.zeros(d)
    mean[7] = 0.25
    s.set_scaling(mean, np.ones(d))
    with pytest.raises(ValueError, match=r"RBL_SCALE_APPLY with centring off .* all-zero mean vector, mean\[7\] is 0.25"):
        s.set_data(A, y, scaling="apply")
    s.set_scaling(np.zeros(d), want)
    s.set_data(A, y, scaling="apply")
    assert np.array_equal(s.get_D(), -y[:, None] * _prescaled(A, want).toarray())
    # a borrower has no data path of its own
    s.gram()
    b =R._solver.Solver(n, d, "erm", reg=0.01, storage="csr", share=s)
    code = b.lib.rbl_set_centering(b._h, 0)
    assert code == L.RBL_ERR_STATE and "this handle borrows its data" in L.last_error()
    b.close()
    s.set_data(A, y, scaling="fit")
    s.close()
    # FIT on an objective-only csr handle: no column form
    o = R._solver.Solver(n, d, "erm", storage="csr", objective_only=True)
    o.set_centering(False)
    with pytest.raises(ValueError, match="RBL_SCALE_FIT on an objective-only handle with RBL_STORE_CSR"):
        o.set_data(A, y, scaling="fit")
    o.set_data(A, y)
    o.close()
    # FIT on a shard stays refused, centring on or off
    X = A.toarray()[:100]
    h = R._solver.Solver(100, d, "erm", reg=0.01, storage="f64", n_total=n, row_offset=0)
    h.set_centering(False)
    with pytest.raises(ValueError, match="RBL_SCALE_FIT on a row-sharded handle"):
        h.set_data(X, y[:100], scaling="fit")
    h.set_scaling(np.zeros(d), want)
    h.set_data(X, y[:100], scaling="apply")
    assert np.array_equal(h.get_D(), -y[:100, None] * (X * (1.0 / want)))
    h.close()
