"""GPU checks of the typed data path (include/rbl.h: rbl_set_data_from, rbl_set_scaling, rbl_get_scaling).

* RBL_SCALE_NONE: for every source type {f64, f32, f16} x storage {f64, f32, fp16} x memory {host, device} x row stride
  {d, d + 3}, rbl_get_D is bit for bit the NumPy formula (tests/scaling_ref.py: form_D without a scaling) on the float64
  widening of the same values; so is rbl_set_data (one chunk, five chunks, a row stride beyond d); the fp16 overflow
  refusal reads as on the float64 host route.
* RBL_SCALE_FIT: mean / scale against the two-pass NumPy restatement (tests/scaling_ref.py); D bit-identical to the NumPy
  formula given the returned vectors; everything bit-identical between a host source, a device source and a host
  source uploaded in five chunks.  RBL_SCALE_APPLY, RBL_DATA_ONES_COLUMN, the refusals.
* whole objects (ADMMmethod, OneVsRest, fit_intercept, standardize) on device tensors / float32 arrays against the
  float64 host route, iterate for iterate.
* one matrix of more than 2^32 elements (fp16 source and storage).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import have_gpu
import scaling_ref

pytestmark = pytest.mark.gpu

SRC = {"f64": np.float64, "f32": np.float32, "f16": np.float16}


@pytest.fixture(scope="module")
def R():
    if not have_gpu():
        pytest.skip("no GPU")
    import admm_for_rank_based_loss_amd as rbl
    return rbl


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _labels(rng, n):
    return np.where(rng.random(n) < 0.5, 1.0, -1.0)


def _wide(X, pad, dev, torch):
    """X as the [:, :d] slice of an array / device tensor with `pad` more columns (row stride d + pad)"""
    n, d = X.shape
    W = np.full((n, d + pad), 7.0, dtype=X.dtype)
    W[:, :d] = X
    if dev:
        return torch.from_numpy(W).cuda()[:, :d]
    return W[:, :d]


# ----------------------------------------------------------------------------------------------- RBL_SCALE_NONE
@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (257, 130), (1000, 1001), (4099, 264)])
def test_none_is_bit_identical_to_set_data(R, torch, shape, storage):
    """one packet, a padded tail, rows that are 16-byte aligned (264, all types) and rows that are not (1001 in fp32 /
    fp16; 130 in fp16), more rows than one block.  The reference is the NumPy formula: rbl_set_data is this very path
    with a float64 host source (its own tests are below)"""
    n, d = shape
    rng = np.random.default_rng(n * 1000 + d)
    X64 = rng.standard_normal((n, d))
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
    for name, dt in SRC.items():
        X = X64.astype(dt)
        ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, storage)    # the widened values, rounded once
        for dev in (False, True):
            for pad in (0, 3):
                src = _wide(X, pad, dev, torch) if pad else (torch.from_numpy(X).cuda() if dev else X)
                got_src = R._solver.as_source(src, 0)
                assert got_src.ldx == (d + pad if n > 1 else d)         # (one row has no stride)
                assert got_src.mem == (1 if dev else 0) and got_src.dtype == R._lib.SOURCE_DTYPE[np.dtype(dt)]
                if not dev:
                    assert got_src.ptr == src.ctypes.data      # the caller's own memory
                s.set_data(np.zeros((n, d)), y)                 # (so that a call that wrote nothing cannot pass)
                s.set_data(src, y)
                assert _same(s.get_D(), ref), (name, storage, "device" if dev else "host", pad)
    s.close()


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_none_on_a_slice_with_a_misaligned_base(R, torch, name):
    rng = np.random.default_rng(11)
    T = torch.from_numpy(rng.standard_normal((258, 130)).astype(SRC[name])).cuda()
    V = T[1:, 1:]                                        # base 131 elements in: not 16-byte aligned, row stride 130
    assert V.data_ptr() % 16 != 0
    n, d = V.shape
    y = _labels(rng, n)
    for storage in ("f64", "f32", "fp16"):
        s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
        ref = scaling_ref.form_D(V.cpu().numpy().astype(np.float64), y, None, None, storage)
        s.set_data(V, y)
        assert _same(s.get_D(), ref), storage
        s.close()


# ------------------------------------------------------------------------- rbl_set_data, the float64 host route
F64_SHAPES = [(1, 1), (3, 5), (257, 130), (1000, 1001)]


@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
@pytest.mark.parametrize("shape", F64_SHAPES)
def test_set_data_f64_is_the_numpy_formula(R, shape, storage):
    """one packet, a padded tail, rows that are no multiple of 16 bytes (1001 doubles: the element-wise loads), more
    rows than one block"""
    n, d = shape
    rng = np.random.default_rng(n * 1000 + d + 1)
    X = rng.standard_normal((n, d))
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
    s.set_data(np.zeros((n, d)), y)
    s.set_data_f64(X, y)
    assert _same(s.get_D(), scaling_ref.form_D(X, y, None, None, storage))
    s.close()


@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
def test_set_data_f64_in_five_chunks(R, storage, monkeypatch):
    """1024 rows a chunk at 4099 x 264: both staging buffers are used twice, the copy of chunk 2 waits for chunk 0's
    kernel"""
    n, d = 4099, 264
    rng = np.random.default_rng(13)
    X = rng.standard_normal((n, d))
    y = _labels(rng, n)
    out = []
    for chunk_bytes in (None, 1024 * 264 * 8):
        monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
        if chunk_bytes:
            monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", str(chunk_bytes))
        s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
        s.set_data(np.zeros((n, d)), y)
        s.set_data_f64(X, y)
        out.append(s.get_D())
        s.close()
    monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
    assert _same(out[1], out[0])
    assert _same(out[1], scaling_ref.form_D(X, y, None, None, storage))


@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
def test_rbl_set_data_with_a_row_stride_beyond_d(R, storage):
    """ldx = d + 3: the rows of the [:, :d] view of a C-contiguous 257 x 133 array (7.0 beyond column 130); the view's
    last row ends three elements before the array does, and nothing beyond column d is read into D"""
    L = R._lib
    n, d, pad = 257, 130, 3
    rng = np.random.default_rng(17)
    W = np.full((n, d + pad), 7.0)
    W[:, :d] = rng.standard_normal((n, d))
    V = W[:, :d]
    assert W.flags["C_CONTIGUOUS"] and V.strides == ((d + pad) * 8, 8)
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
    s.set_data(np.zeros((n, d)), y)
    L.check(s.lib.rbl_set_data(s._h, C.c_void_p(V.ctypes.data), L.ptr(y), d + pad))
    assert _same(s.get_D(), scaling_ref.form_D(V, y, None, None, storage))
    s.close()


def test_fp16_overflow_reads_as_on_the_float64_host_route(R, torch):
    rng = np.random.default_rng(2)
    n, d = 300, 41
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[7, 40] = 70000.0
    X[150, 3] = -70000.0
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage="fp16")
    with pytest.raises(ValueError) as host:
        s.set_data_f64(X.astype(np.float64), y)
    assert "fp16 storage: 2 finite entries do not fit float16" in str(host.value) and "first at row 7, column 40" in str(host.value)
    for src in (torch.from_numpy(X).cuda(), X):
        with pytest.raises(ValueError) as e:
            s.set_data(src, y)
        assert str(e.value) == str(host.value)
        with pytest.raises(Exception):                   # the handle is left without data
            s.step(False)
    s.close()


# ------------------------------------------------------------------------------------------------ RBL_SCALE_FIT
def _fit_matrix(name):
    """4099 x 9: a column whose mean dwarfs its spread (mean 1e6, unit spread; float16 cannot hold 1e6: mean 1000 there),
    a constant column, a column of +-65000 (fits float16 raw), the rest standard normal"""
    rng = np.random.default_rng(9)
    n, d = 4099, 9
    X = rng.standard_normal((n, d))
    X[:, 0] += 1000.0 if name == "f16" else 1e6
    X[:, 1] = 2.5
    X[:, 2] = np.where(rng.random(n) < 0.5, 65000.0, -65000.0)
    return X.astype(SRC[name]), _labels(rng, n)


@pytest.mark.parametrize("name", ["f64", "f32", "f16"])
def test_fit_statistics_and_matrix(R, torch, name, monkeypatch):
    X, y = _fit_matrix(name)
    n, d = X.shape
    Xw = X.astype(np.float64)
    mean_ref, scale_ref = scaling_ref.fit(Xw)
    Xdev = torch.from_numpy(X).cuda()
    first = None
    for storage in ("f64", "f32", "fp16"):
        out = []
        for how in ("host", "device", "chunks"):
            monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
            if how == "chunks":                          # 1024 rows a chunk: five chunks at this size
                monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", str(1024 * d * X.itemsize))
            s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
            assert s.get_scaling() is None
            s.set_data(Xdev if how == "device" else X, y, scaling="fit")
            mean, scale = s.get_scaling()
            out.append((mean, scale, s.get_D()))
            s.close()
        monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
        mean, scale, D = out[0]
        # 1e-12 relative: the scale against the scale, the mean against |mean| + scale.  (A mean is only defined to about
        # eps * scale - the two-pass NumPy sum has that error itself - so for the standard normal columns, whose means
        # are 1e-4 .. 1e-2, a bound relative to |mean| alone would measure the reference's rounding: on the MI355X the
        # two differ by 3.7e-16 absolute on a mean of 2.6e-4, 1.5e-12 of the mean and 3.7e-16 of the scale.)
        print(name, storage, "max |dmean| / (|mean| + scale):", np.max(np.abs(mean - mean_ref) / (np.abs(mean_ref) + scale_ref)),
              "max |dscale| / scale:", np.max(np.abs(scale - scale_ref) / scale_ref))
        assert np.all(np.abs(mean - mean_ref) <= 1e-12 * (np.abs(mean_ref) + scale_ref))
        assert np.all(np.abs(scale - scale_ref) <= 1e-12 * scale_ref)
        assert scale[1] == 1.0 and mean[1] == 2.5       # the constant column
        # given the returned vectors the matrix is the NumPy formula, bit for bit
        assert _same(D, scaling_ref.form_D(Xw, y, mean, scale, storage)), storage
        assert np.all(D[:, 1] == 0.0)
        for other in out[1:]:                            # host = device = host in five chunks
            assert _same(other[0], mean) and _same(other[1], scale) and _same(other[2], D), storage
        if first is None:
            first = (mean, scale)
        assert _same(first[0], mean) and _same(first[1], scale)      # (the statistics do not depend on the storage type)


def test_fit_names_a_column_with_a_non_finite_statistic(R):
    X = np.random.default_rng(0).standard_normal((50, 4)).astype(np.float32)
    X[20, 2] = np.inf
    s = R.Solver(50, 4, "erm", reg=0.1, storage="f32", objective_only=True)
    with pytest.raises(ValueError, match="column 2 has a non-finite"):
        s.set_data(X, np.ones(50), scaling="fit")
    s.close()


def test_apply_on_a_test_matrix(R, torch):
    X, y = _fit_matrix("f32")
    mean, scale = scaling_ref.fit(X.astype(np.float64))
    Xt, yt = X[:513], y[:513]
    for storage in ("f64", "f32", "fp16"):
        for src in (Xt, torch.from_numpy(Xt).cuda()):
            t = R.Solver(513, 9, "erm", reg=0.1, storage=storage, objective_only=True)
            with pytest.raises(R._lib.RblError, match="RBL_SCALE_APPLY without a scaling") as e:
                t.set_data(src, yt, scaling="apply")
            assert e.value.code == R._lib.RBL_ERR_STATE
            t.set_scaling(mean, scale)
            got = t.get_scaling()
            assert _same(got[0], mean) and _same(got[1], scale)
            t.set_data(src, yt, scaling="apply")
            assert _same(t.get_D(), scaling_ref.form_D(Xt.astype(np.float64), yt, mean, scale, storage)), storage
            t.set_scaling(None, None)
            assert t.get_scaling() is None
            t.close()


def test_ones_column(R, torch):
    rng = np.random.default_rng(4)
    n, d = 257, 130
    X = rng.standard_normal((n, d)).astype(np.float32)
    y = _labels(rng, n)
    for storage in ("f64", "f32", "fp16"):
        s = R.Solver(n, d + 1, "erm", reg=0.1, storage=storage, objective_only=True)
        ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, storage, ones_column=True)
        for src in (X, torch.from_numpy(X).cuda()):
            s.set_data(np.zeros((n, d + 1)), y)
            s.set_data(src, y, ones_column=True)
            assert _same(s.get_D(), ref), storage
            s.set_data(src, y, scaling="fit", ones_column=True)
            mean, scale = s.get_scaling()
            assert (mean[d], scale[d]) == (0.0, 1.0)
            assert _same(s.get_D(), scaling_ref.form_D(X.astype(np.float64), y, mean[:d], scale[:d], storage, ones_column=True))
        with pytest.raises(ValueError, match="expected"):
            s.set_data(X, y)                             # d columns into a handle of d + 1 without the flag
        s.close()


def test_refusals(R, torch):
    L = R._lib
    lib = L.load()
    rng = np.random.default_rng(6)
    n, d = 64, 5
    X = rng.standard_normal((n, d))
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True)

    def call(ptr, dtype=L.DTYPE_F64, mem=L.MEM_HOST, ldx=d, yy=y, scaling=0, flags=0, h=None):
        return lib.rbl_set_data_from((h or s)._h, C.c_void_p(ptr), dtype, mem, ldx, L.ptr(yy), scaling, flags)

    # a host pointer passed as device memory: refused with a message, nothing is launched on it
    assert call(X.ctypes.data, mem=L.MEM_DEVICE) == L.RBL_ERR_INVALID
    assert "not device memory" in L.last_error()
    assert call(X.ctypes.data, ldx=d - 1) == L.RBL_ERR_INVALID and "ldx=4" in L.last_error()
    assert call(X.ctypes.data, ldx=d - 2, flags=L.DATA_ONES_COLUMN) == L.RBL_ERR_INVALID
    assert call(X.ctypes.data, dtype=3) == L.RBL_ERR_INVALID and "dtype" in L.last_error()
    assert call(X.ctypes.data, mem=2) == L.RBL_ERR_INVALID and "memory kind" in L.last_error()
    assert call(X.ctypes.data, scaling=3) == L.RBL_ERR_INVALID and "scaling" in L.last_error()
    assert call(X.ctypes.data, flags=2) == L.RBL_ERR_INVALID and "flags" in L.last_error()
    assert call(None) == L.RBL_ERR_INVALID and "X NULL" in L.last_error()
    assert lib.rbl_set_data_from(s._h, C.c_void_p(X.ctypes.data), 0, 0, d, None, 0, 0) == L.RBL_ERR_INVALID
    assert call(X.ctypes.data, yy=np.full(n, 0.5)) == L.RBL_ERR_INVALID and "+1/-1" in L.last_error()
    with pytest.raises(ValueError, match="scale"):
        s.set_scaling(np.zeros(d), np.zeros(d))
    with pytest.raises(ValueError, match="scaling must be one of"):
        s.set_data(X, y, scaling="both")
    with pytest.raises(Exception):                       # none of the refused calls left data behind
        s.risk(np.zeros(d))
    assert call(X.ctypes.data) == L.RBL_OK               # and the handle still works
    # RBL_SCALE_FIT on a row shard: the message points to APPLY
    shard = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True, n_total=2 * n, row_offset=0)
    with pytest.raises(ValueError, match="row-sharded handle.*RBL_SCALE_APPLY"):
        shard.set_data(X, y, scaling="fit")
    mean, scale = scaling_ref.fit(X)
    shard.set_scaling(mean, scale)
    shard.set_data(X, y, scaling="apply")                # what a shard does instead
    assert _same(shard.get_D(), scaling_ref.form_D(X, y, mean, scale, "f32"))
    shard.close()
    # a borrower has no data path of its own
    bor = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True, share=s)
    for src in (X, torch.from_numpy(X).cuda()):
        with pytest.raises(L.RblError, match="borrows its data") as e:
            bor.set_data(src, y)
        assert e.value.code == L.RBL_ERR_STATE
    bor.close()
    # a tensor of a type without an instance never reaches the library
    with pytest.raises(ValueError, match="float64, float32 and float16"):
        s.set_data(torch.zeros(n, d, dtype=torch.bfloat16, device="cuda"), y)
    s.close()


# ------------------------------------------------------------------------------------------------- whole objects
KW = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])


@pytest.fixture(scope="module")
def problem(torch):
    rng = np.random.default_rng(21)
    n, d = 2000, 60
    X = (rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, d) + rng.uniform(-2.0, 2.0, d)).astype(np.float32)
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.where(X.astype(np.float64) @ w + 0.5 * rng.standard_normal(n) > 0, 1.0, -1.0)
    lab = rng.integers(0, 3, n)
    return X, y, lab, torch.from_numpy(X).cuda()


def _state(s):
    st = s._s.get_state()
    return st["w"], st["z"], st["lam"]


@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_admm_on_a_device_tensor_matches_the_float64_host_route(R, problem, storage):
    X, y, _, Xc = problem
    a = R.ADMMmethod(Xc, y, max_iter=10, tol=0, storage=storage, **KW)
    b = R.ADMMmethod(Xc.cpu().double().numpy(), y, max_iter=10, tol=0, storage=storage, **KW)
    assert _same(a._s.get_D(), b._s.get_D())
    a.main_loop(verbose=False)
    b.main_loop(verbose=False)
    for u, v in zip(_state(a), _state(b)):
        assert _same(u, v)
    assert a.scale_mean_ is None and a.unscaled()[1] == 0.0


def test_one_vs_rest_on_a_device_tensor(R, problem):
    X, _, lab, Xc = problem
    kw = dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.01, max_iter=10, tol=0, storage="f32")
    a = R.OneVsRest(Xc, lab, **kw)
    b = R.OneVsRest(X.astype(np.float64), lab, **kw)
    Wa, Wb = a.main_loop(verbose=False), b.main_loop(verbose=False)
    assert Wa.shape == (60, 3) and _same(Wa, Wb)
    assert np.array_equal(a.predict(Xc[:500]), b.predict(X[:500].astype(np.float64)))
    a.close()
    b.close()


def test_fit_intercept_without_a_host_copy(R, problem):
    X, y, _, Xc = problem
    ref = R.ADMMmethod(X.astype(np.float64), y, max_iter=10, tol=0, storage="f32", fit_intercept=True, **KW)
    D_ref = ref._s.get_D()
    assert D_ref.shape == (2000, 61) and np.array_equal(D_ref[:, 60], -y)
    # (all three exist before any of them iterates: how the w-step is launched depends on the handles alive beside it)
    others = [R.ADMMmethod(src, y, max_iter=10, tol=0, storage="f32", fit_intercept=True, **KW) for src in (X, Xc)]
    ref.main_loop(verbose=False)
    for a in others:
        assert _same(a._s.get_D(), D_ref)
        a.main_loop(verbose=False)
        for u, v in zip(_state(a), _state(ref)):
            assert _same(u, v)


@pytest.mark.parametrize("storage", ["f32", "fp16"])
def test_standardize(R, problem, storage):
    X, y, _, Xc = problem
    Xw = X.astype(np.float64)
    Xt, yt = Xc[:700], y[:700]
    a = R.ADMMmethod(Xc, y, max_iter=10, tol=0, storage=storage, standardize=True, fit_intercept=True, **KW)
    mean, scale = a.scale_mean_, a.scale_scale_
    assert mean.shape == scale.shape == (60,)
    mr, sr = scaling_ref.fit(Xw)
    assert np.allclose(mean, mr, rtol=1e-12, atol=1e-12) and np.allclose(scale, sr, rtol=1e-12, atol=0)
    # the solve on the host-standardised matrix (formed with the returned vectors) is the same solve
    Z = scaling_ref.standardize(Xw, mean, scale)
    b = R.ADMMmethod(Z, y, max_iter=10, tol=0, storage=storage, fit_intercept=True, **KW)
    assert _same(a._s.get_D(), b._s.get_D())
    a.start_store(Xt, yt, **KW)
    b.start_store(Z[:700], yt, **KW)
    c = R.ADMMmethod(Xw, y, max_iter=10, tol=0, storage=storage, standardize=True, fit_intercept=True, **KW)   # the host route
    c.start_store(Xw[:700], yt, **KW)
    for s in (a, b, c):
        s.main_loop(verbose=False)
    for u, v, w_ in zip(_state(a), _state(b), _state(c)):
        assert _same(u, v) and _same(u, w_)
    assert len(a.test_losses) == 11 and a.test_losses == b.test_losses == c.test_losses
    # a solver that borrows standardised data says so itself, or is refused
    with pytest.raises(ValueError, match="share_data holds standardised data"):
        R.ADMMmethod(Xc, y, max_iter=10, tol=0, storage=storage, fit_intercept=True, share_data=a, **KW)
    # unscaled(): the same scores on raw rows
    coef, icpt = a.unscaled()
    w = a.w.reshape(-1)
    assert np.max(np.abs((Xw @ coef + icpt) - (Z @ w[:60] + w[60]))) <= 1e-10
    # the mirrors of the reference's metrics take the scaling through their optional argument
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
    acc = calculate_accuracy(w, Xt, yt, scaling=(mean, scale))
    assert acc == calculate_accuracy(w, np.hstack([Z[:700], np.ones((700, 1))]), yt)


# ------------------------------------------------------------------------------------------- beyond 2^32 elements
def test_more_than_2_to_32_elements(R, torch):
    """fp16 source and storage, 4 300 000 x 1000 (8.6 GB each): the rows beyond element 2^32 are formed like the first"""
    n, d, tail = 4_300_000, 1000, 8192
    assert n * d > 2 ** 32
    if torch.cuda.mem_get_info()[0] < 40 * 2 ** 30:
        pytest.skip("needs 40 GB of free device memory")
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, n, 100_000):                      # (in pieces: no fp32 copy of the whole matrix)
        r1 = min(n, r0 + 100_000)
        X[r0:r1] = torch.randn((r1 - r0, d), generator=g, device="cuda").half()
    w = np.random.default_rng(8).standard_normal(d)
    s = R.Solver(n, d, "erm", storage="fp16", objective_only=True)
    s.set_data(X, np.ones(n))
    cls = s.decide_multi(np.stack([w, -w]))
    s.close()
    xw = (X[n - tail:].double() @ torch.from_numpy(w).cuda()).cpu().numpy()
    del X
    keep = np.abs(xw) >= 1e-2
    assert np.mean(~keep) <= 0.01, np.mean(~keep)
    assert np.array_equal(cls[n - tail:][keep] == 0, xw[keep] > 0)
    assert 0.4 < np.mean(cls == 0) < 0.6                 # and the rows before them are not all one class
