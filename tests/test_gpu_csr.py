"""GPU checks of the sparse data path (include/rbl.h: rbl_set_data_csr): CSR arrays, on the host or on the solver's GPU,
expanded on the device into the dense chunks that the typed data path (rbl_set_data_from) reads.

* RBL_SCALE_NONE: values {f64, f32, f16} x storage {f64, f32, fp16} x memory {host, device} x indices {int32, int64}:
  rbl_get_D is bit for bit the NumPy formula (tests/scaling_ref.py: form_D) on the widened dense expansion.
* row patterns in one matrix (empty rows, single entries at both ends, a full row, rows around one wave's width, explicit
  zeros and -0.0), and nnz == 0 with NULL arrays - against the formula and against the dense route itself.
* RBL_SCALE_FIT / APPLY / RBL_DATA_ONES_COLUMN: vectors and D bit-identical to the dense source's, and between a host
  source, a device source and a host source in five chunks.
* the refusals: each is RBL_ERR_INVALID with its message, leaves the handle without data, and a valid call then works.
* whole objects on sparse input against the same objects on toarray(), iterate for iterate."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import have_gpu
import scaling_ref

pytestmark = pytest.mark.gpu

sp = pytest.importorskip("scipy.sparse")

SRC = {"f64": np.float64, "f32": np.float32, "f16": np.float16}
IDX = {"i32": np.int32, "i64": np.int64}


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


def _csr_arrays(X):
    """(indptr, indices, data) of the non-zero entries of the dense X, in X's type, int64 indices"""
    A = sp.csr_matrix(X.astype(np.float64))
    A.sort_indices()
    r = np.repeat(np.arange(X.shape[0]), np.diff(A.indptr))
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(X[r, A.indices])


def _dense(shape, indptr, indices, data):
    """the dense expansion: implicit entries +0.0, stored entries with their bits"""
    A = np.zeros(shape, dtype=data.dtype)
    r = np.repeat(np.arange(shape[0]), np.diff(indptr))
    A[r, indices] = data
    return A


def _source(R, torch, shape, indptr, indices, data, itype, dev):
    """a CsrSource on exactly these arrays (any value type, float16 included), on the host or on the device"""
    L = R._lib
    ip, ix, vl = (np.ascontiguousarray(indptr, dtype=itype), np.ascontiguousarray(indices, dtype=itype),
                  np.ascontiguousarray(data))
    if dev:
        keep = [torch.from_numpy(a).cuda() for a in (ip, ix, vl)]
        torch.cuda.synchronize()
        ptrs = [t.data_ptr() for t in keep]
    else:
        keep = [ip, ix, vl]
        ptrs = [a.ctypes.data for a in keep]
    return R._solver.CsrSource(shape, L.SOURCE_DTYPE[vl.dtype], L.MEM_DEVICE if dev else L.MEM_HOST,
                               L.INDEX_DTYPE[np.dtype(itype)], vl.shape[0], ptrs[0], ptrs[1], ptrs[2], keep)


def _sparse_normal(rng, n, d, density):
    X = rng.standard_normal((n, d))
    X[rng.random((n, d)) >= density] = 0.0
    if n * d > 1:
        X[n // 2, d // 2] = 1.25                         # (never all zero)
    else:
        X[0, 0] = -0.75
    return X


# ----------------------------------------------------------------------------------------------- RBL_SCALE_NONE
@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (257, 130), (1000, 1001), (4099, 264)])
def test_none_is_bit_identical_to_the_dense_formula(R, torch, shape, storage):
    n, d = shape
    rng = np.random.default_rng(n * 1000 + d + 7)
    X64 = _sparse_normal(rng, n, d, 0.15)
    y = _labels(rng, n)
    s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
    for name, dt in SRC.items():
        X = X64.astype(dt)
        indptr, indices, data = _csr_arrays(X)
        assert data.dtype == np.dtype(dt) and np.array_equal(_dense(shape, indptr, indices, data), X)
        ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, storage)
        for dev in (False, True):
            for iname, itype in IDX.items():
                src = _source(R, torch, shape, indptr, indices, data, itype, dev)
                s.set_data(np.zeros((n, d)), y)             # (so that a call that wrote nothing cannot pass)
                s.set_data(src, y)
                assert _same(s.get_D(), ref), (name, storage, "device" if dev else "host", iname)
    s.close()


def _pattern_matrix():
    """300 x 1001: an empty first row, an empty last row, a run of empty rows, single entries at column 0 and at column
    ds - 1, a full row, rows of 63 / 64 / 65 entries (one wave's width), a row of 257, explicit zeros and -0.0"""
    rng = np.random.default_rng(31)
    n, d = 300, 1001
    rows = {}
    rows[1] = np.array([0])
    rows[2] = np.array([d - 1])
    rows[3] = np.array([0, d - 1])
    rows[10] = np.arange(d)
    for r, k in ((20, 63), (21, 64), (22, 65), (23, 257), (24, 128), (25, 1)):
        rows[r] = np.sort(rng.choice(d, k, replace=False))
    for r in range(60, 299):                              # (rows 30 .. 59 and 299 stay empty)
        rows[r] = np.sort(rng.choice(d, int(rng.integers(0, 40)), replace=False))
    indptr = np.zeros(n + 1, dtype=np.int64)
    for r in range(n):
        indptr[r + 1] = indptr[r] + (len(rows[r]) if r in rows else 0)
    indices = np.concatenate([rows[r] for r in sorted(rows)]).astype(np.int64)
    data = rng.standard_normal(indices.shape[0])
    data[rng.random(data.shape[0]) < 0.05] = 0.0          # explicit zeros
    data[rng.random(data.shape[0]) < 0.05] = -0.0         # and negative zeros: the bits are copied
    a = indptr[22]
    data[a], data[a + 1] = 0.0, -0.0
    assert indptr[1] == 0 and indptr[n] == indptr[n - 1] and np.all(np.diff(indptr[30:61]) == 0)
    return (n, d), indptr, indices, data, _labels(rng, n)


@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
def test_row_patterns(R, torch, storage):
    shape, indptr, indices, data64, y = _pattern_matrix()
    n, d = shape
    s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
    for name, dt in SRC.items():
        data = data64.astype(dt)
        A = _dense(shape, indptr, indices, data)
        assert np.signbit(A).sum() > np.sum(A < 0)        # some -0.0 made it into the expansion
        ref = scaling_ref.form_D(A.astype(np.float64), y, None, None, storage)
        s.set_data(A, y)                                  # the dense route itself
        assert _same(s.get_D(), ref), (name, storage)
        for dev in (False, True):
            for itype in IDX.values():
                s.set_data(np.zeros((n, d)), y)
                s.set_data(_source(R, torch, shape, indptr, indices, data, itype, dev), y)
                assert _same(s.get_D(), ref), (name, storage, dev, itype)
    s.close()


def test_no_entries_at_all_with_null_arrays(R, torch):
    L = R._lib
    lib = L.load()
    n, d = 70, 9
    y = _labels(np.random.default_rng(1), n)
    s = R.Solver(n, d + 1, "erm", reg=0.1, storage="f32", objective_only=True)
    for dev in (False, True):
        for itype, it in ((np.int32, L.INDEX_I32), (np.int64, L.INDEX_I64)):
            ip = np.zeros(n + 1, dtype=itype)
            keep = torch.from_numpy(ip).cuda() if dev else ip
            p = keep.data_ptr() if dev else ip.ctypes.data
            s.set_data(np.ones((n, d + 1)), y)
            rc = lib.rbl_set_data_csr(s._h, C.c_void_p(p), None, None, 0, it, L.DTYPE_F32, L.MEM_DEVICE if dev else L.MEM_HOST,
                                      L.ptr(y), 0, L.DATA_ONES_COLUMN)
            assert rc == L.RBL_OK, L.last_error()
            assert _same(s.get_D(), scaling_ref.form_D(np.zeros((n, d)), y, None, None, "f32", ones_column=True))
    # SciPy's empty matrix goes the same way
    s.set_data(np.ones((n, d + 1)), y)
    s.set_data(sp.csr_matrix((n, d), dtype=np.float64), y, ones_column=True)
    assert _same(s.get_D(), scaling_ref.form_D(np.zeros((n, d)), y, None, None, "f32", ones_column=True))
    s.close()


# ------------------------------------------------------------------------------------- RBL_SCALE_FIT / APPLY / ones
def _fit_matrix(name):
    """4099 x 9, density 0.3: a column whose mean dwarfs its spread once it is dense (explicit entries everywhere), a
    constant column (every entry explicit), a column without any entry, a column of +-65000 entries"""
    rng = np.random.default_rng(9)
    n, d = 4099, 9
    X = rng.standard_normal((n, d))
    X[rng.random((n, d)) >= 0.3] = 0.0
    X[:, 0] = rng.standard_normal(n) + (1000.0 if name == "f16" else 1e6)
    X[:, 1] = 2.5
    X[:, 2] = np.where(rng.random(n) < 0.5, 65000.0, -65000.0) * (rng.random(n) < 0.3)
    X[:, 3] = 0.0
    X[0, 4:] = 0.0                                        # (the shift row has implicit entries)
    X += 0.0                                              # (-65000 * False is -0.0: an implicit entry is +0.0)
    return X.astype(SRC[name]), _labels(rng, n)


def _ldc(d, itemsize):
    per = 16 // itemsize
    return -(-d // per) * per


@pytest.mark.parametrize("name", ["f64", "f32", "f16"])
def test_fit_is_bit_identical_to_the_dense_source(R, torch, name, monkeypatch):
    X, y = _fit_matrix(name)
    n, d = X.shape
    indptr, indices, data = _csr_arrays(X)
    Xw = X.astype(np.float64)
    for storage in ("f64", "f32", "fp16"):
        monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
        s = R.Solver(n, d, "erm", reg=0.1, storage=storage, objective_only=True)
        s.set_data(X, y, scaling="fit")                  # the dense source: the yardstick
        mean, scale = s.get_scaling()
        D = s.get_D()
        assert scale[1] == 1.0 and mean[1] == 2.5 and np.all(D[:, 1] == 0.0)     # the constant column
        assert scale[3] == 1.0 and mean[3] == 0.0 and np.all(D[:, 3] == 0.0)     # the column without entries
        assert _same(D, scaling_ref.form_D(Xw, y, mean, scale, storage))
        for how in ("host", "device", "chunks"):
            monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
            if how == "chunks":                          # 1024 dense staging rows a chunk: five chunks at this size
                monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", str(1024 * _ldc(d, X.itemsize) * X.itemsize))
            for itype in IDX.values():
                s.set_scaling(None, None)
                s.set_data(np.zeros((n, d)), y)
                s.set_data(_source(R, torch, X.shape, indptr, indices, data, itype, how == "device"), y, scaling="fit")
                m2, s2 = s.get_scaling()
                assert _same(m2, mean) and _same(s2, scale) and _same(s.get_D(), D), (name, storage, how, itype)
        monkeypatch.delenv("RBL_UPLOAD_CHUNK_BYTES", raising=False)
        s.close()


def test_none_in_five_chunks(R, torch, monkeypatch):
    """without FIT the chunks are no whole row blocks: 820 rows a chunk at 4099 x 264, both sets of slices used twice"""
    rng = np.random.default_rng(12)
    n, d = 4099, 264
    X = _sparse_normal(rng, n, d, 0.1).astype(np.float32)
    X[820:1640] = 0.0                                     # one chunk without a single entry
    y = _labels(rng, n)
    indptr, indices, data = _csr_arrays(X)
    monkeypatch.setenv("RBL_UPLOAD_CHUNK_BYTES", str(820 * d * 4))
    s = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True)
    ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, "f32")
    for dev in (False, True):
        s.set_data(np.zeros((n, d)), y)
        s.set_data(_source(R, torch, X.shape, indptr, indices, data, np.int32, dev), y)
        assert _same(s.get_D(), ref), dev
    s.close()


def test_apply_and_ones_column(R, torch):
    X, y = _fit_matrix("f32")
    n, d = X.shape
    mean, scale = scaling_ref.fit(X.astype(np.float64))
    Xt, yt = X[:513], y[:513]
    indptr, indices, data = _csr_arrays(Xt)
    for storage in ("f64", "f32", "fp16"):
        for dev in (False, True):
            src = _source(R, torch, Xt.shape, indptr, indices, data, np.int32, dev)
            t = R.Solver(513, d, "erm", reg=0.1, storage=storage, objective_only=True)
            with pytest.raises(R._lib.RblError, match="RBL_SCALE_APPLY without a scaling") as e:
                t.set_data(src, yt, scaling="apply")
            assert e.value.code == R._lib.RBL_ERR_STATE
            t.set_scaling(mean, scale)
            t.set_data(src, yt, scaling="apply")
            assert _same(t.get_D(), scaling_ref.form_D(Xt.astype(np.float64), yt, mean, scale, storage)), storage
            t.close()
            # the column of ones: never scaled, reported as (0, 1)
            o = R.Solver(513, d + 1, "erm", reg=0.1, storage=storage, objective_only=True)
            o.set_data(Xt, yt, scaling="fit", ones_column=True)
            m1, s1 = o.get_scaling()
            D1 = o.get_D()
            o.set_scaling(None, None)
            o.set_data(np.zeros((513, d + 1)), yt)
            o.set_data(src, yt, scaling="fit", ones_column=True)
            m2, s2 = o.get_scaling()
            assert (m2[d], s2[d]) == (0.0, 1.0) and _same(m1, m2) and _same(s1, s2) and _same(o.get_D(), D1)
            if storage == "fp16":                        # column 0 (1e6) does not fit unscaled: refused as on the dense route
                with pytest.raises(ValueError, match="513 finite entries do not fit float16.*first at row 0, column 0"):
                    o.set_data(src, yt, ones_column=True)
            else:
                o.set_data(src, yt, ones_column=True)
                assert _same(o.get_D(), scaling_ref.form_D(Xt.astype(np.float64), yt, None, None, storage, ones_column=True))
            with pytest.raises(ValueError, match="expected"):
                o.set_data(src, yt)                      # d columns into a handle of d + 1 without the flag
            o.close()


# ------------------------------------------------------------------------------------------------------ refusals
def _refusal_case():
    rng = np.random.default_rng(6)
    n, d = 64, 40
    X = _sparse_normal(rng, n, d, 0.3).astype(np.float32)
    X[30] = 0.0
    X[30, [3, 9, 17, 25]] = [1.0, 2.0, 3.0, 4.0]          # the middle row every bad index goes into
    X[n - 1, 5] = 1.0                                     # (the last row is not empty)
    return X, _labels(rng, n)


def _call(R, s, indptr, indices, data, itype, mem, y, scaling=0, ptrs=None):
    L = R._lib
    ip, ix, vl = np.ascontiguousarray(indptr, dtype=itype), np.ascontiguousarray(indices, dtype=itype), np.ascontiguousarray(data)
    p = ptrs or [a.ctypes.data for a in (ip, ix, vl)]
    return L.load().rbl_set_data_csr(s._h, C.c_void_p(p[0]), C.c_void_p(p[1]), C.c_void_p(p[2]), vl.shape[0],
                                     L.INDEX_DTYPE[np.dtype(itype)], L.SOURCE_DTYPE[vl.dtype], mem, L.ptr(y), scaling, 0)


def _stepped(R, s):
    st = R._lib.RblStats()
    return R._lib.load().rbl_step(s._h, 0, C.byref(st))


ENTRY_CASES = {          # the four entries of row 30 are replaced; ds = 40, so every |index| < 2 ds
    "minus_one": ([-1, 9, 17, 25], r"row 30: column index -1 .* outside \[0, 40\)"),
    "equal_to_ds": ([3, 9, 17, 40], r"row 30: column index 40 .* outside \[0, 40\)"),
    "equal_pair": ([3, 9, 9, 25], r"row 30: column index 9 is repeated .*coalesce"),
    "descending_pair": ([3, 17, 9, 25], r"row 30: column index 9 follows 17 .*strictly increasing.*coalesce"),
}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("itype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", sorted(ENTRY_CASES))
def test_entry_refusals(R, torch, case, itype, dev):
    """the expand kernel refuses the entry (it is not written), the call fails after the first pass over the source -
    the statistics pass under FIT, else the forming pass - and the handle is left without data"""
    L = R._lib
    X, y = _refusal_case()
    n, d = X.shape
    indptr, indices, data = _csr_arrays(X)
    a = indptr[30]
    assert indptr[31] - a == 4
    bad = indices.copy()
    bad[a:a + 4] = ENTRY_CASES[case][0]
    ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, "f32")
    for scaling in (0, 1):
        s = R.Solver(n, d, "erm", reg=0.1, storage="f32")
        good = _source(R, torch, X.shape, indptr, indices, data, itype, dev)
        s.set_data(good, y)                               # the handle holds data ...
        src = _source(R, torch, X.shape, indptr, bad, data, itype, dev)
        rc = L.load().rbl_set_data_csr(s._h, C.c_void_p(src.indptr), C.c_void_p(src.indices), C.c_void_p(src.values), src.nnz,
                                       src.index_type, src.dtype, src.mem, L.ptr(y), scaling, 0)
        assert rc == L.RBL_ERR_INVALID
        assert re.search(ENTRY_CASES[case][1], L.last_error()), L.last_error()
        assert _stepped(R, s) == L.RBL_ERR_STATE          # ... and is left without it
        assert s.get_scaling() is None                    # (a failed FIT leaves no vectors behind)
        s.set_data(good, y)                               # a valid call then works
        assert _same(s.get_D(), ref)
        s.close()


def test_structure_refusals(R, torch):
    L = R._lib
    X, y = _refusal_case()
    n, d = X.shape
    indptr, indices, data = _csr_arrays(X)
    ref = scaling_ref.form_D(X.astype(np.float64), y, None, None, "f32")
    dec = indptr.copy()
    dec[31] = dec[30] - 1                                 # row 30 ends before it starts
    first = indptr.copy()
    first[0] = 1
    last = indptr.copy()
    last[n] -= 1
    cases = [(dec, "indptr decreases at row 30"), (first, r"indptr\[0\] is 1, not 0"), (last, r"indptr\[n\] is \d+, nnz is \d+")]
    for itype in (np.int32, np.int64):
        for dev in (False, True):
            for ip, msg in cases:
                s = R.Solver(n, d, "erm", reg=0.1, storage="f32")
                src = _source(R, torch, X.shape, ip, indices, data, itype, dev)
                rc = L.load().rbl_set_data_csr(s._h, C.c_void_p(src.indptr), C.c_void_p(src.indices), C.c_void_p(src.values),
                                               src.nnz, src.index_type, src.dtype, src.mem, L.ptr(y), 0, 0)
                assert rc == L.RBL_ERR_INVALID and re.search(msg, L.last_error()), L.last_error()
                assert _stepped(R, s) == L.RBL_ERR_STATE
                s.set_data(_source(R, torch, X.shape, indptr, indices, data, itype, dev), y)
                assert _same(s.get_D(), ref)
                s.close()
    # a host pointer passed as device memory: refused with a message, nothing is launched on it
    s = R.Solver(n, d, "erm", reg=0.1, storage="f32")
    assert _call(R, s, indptr, indices, data, np.int64, L.MEM_DEVICE, y) == L.RBL_ERR_INVALID
    assert "indptr was passed as RBL_MEM_DEVICE" in L.last_error() and "not device memory" in L.last_error()
    dev_ip = torch.from_numpy(indptr).cuda()
    ix, vl = np.ascontiguousarray(indices), np.ascontiguousarray(data)
    assert _call(R, s, indptr, indices, data, np.int64, L.MEM_DEVICE, y, ptrs=[dev_ip.data_ptr(), ix.ctypes.data, vl.ctypes.data]) \
        == L.RBL_ERR_INVALID
    assert "indices was passed as RBL_MEM_DEVICE" in L.last_error()
    assert _stepped(R, s) == L.RBL_ERR_STATE
    # the arguments
    lib = L.load()
    p = [C.c_void_p(a.ctypes.data) for a in (indptr, ix, vl)]
    assert lib.rbl_set_data_csr(s._h, p[0], p[1], p[2], vl.shape[0], 2, L.DTYPE_F32, 0, L.ptr(y), 0, 0) == L.RBL_ERR_INVALID
    assert "index type" in L.last_error()
    assert lib.rbl_set_data_csr(s._h, p[0], p[1], p[2], vl.shape[0], 1, 3, 0, L.ptr(y), 0, 0) == L.RBL_ERR_INVALID
    assert "dtype" in L.last_error()
    assert lib.rbl_set_data_csr(s._h, p[0], None, p[2], vl.shape[0], 1, L.DTYPE_F32, 0, L.ptr(y), 0, 0) == L.RBL_ERR_INVALID
    assert "indices NULL" in L.last_error()
    assert lib.rbl_set_data_csr(s._h, p[0], C.c_void_p(ix.ctypes.data + 4), p[2], vl.shape[0], 1, L.DTYPE_F32, 0, L.ptr(y), 0, 0) \
        == L.RBL_ERR_INVALID
    assert "aligned" in L.last_error()
    assert _stepped(R, s) == L.RBL_ERR_STATE
    assert _call(R, s, indptr, indices, data, np.int64, L.MEM_HOST, y) == L.RBL_OK       # and the handle still works
    assert _same(s.get_D(), ref)
    # a borrower has no data path of its own
    bor = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True, share=s)
    assert _call(R, bor, indptr, indices, data, np.int64, L.MEM_HOST, y) == L.RBL_ERR_STATE
    assert "borrows its data" in L.last_error()
    bor.close()
    s.close()
    # RBL_SCALE_FIT on a row shard: the message points to APPLY
    shard = R.Solver(n, d, "erm", reg=0.1, storage="f32", objective_only=True, n_total=2 * n, row_offset=0)
    with pytest.raises(ValueError, match="row-sharded handle.*RBL_SCALE_APPLY"):
        shard.set_data(sp.csr_matrix(X), y, scaling="fit")
    with pytest.raises(Exception):
        shard.risk(np.zeros(d))
    shard.set_data(sp.csr_matrix(X), y)
    assert _same(shard.get_D(), ref)
    shard.close()


def test_fp16_overflow_reads_as_on_the_dense_route(R, torch):
    rng = np.random.default_rng(2)
    n, d = 300, 41
    X = _sparse_normal(rng, n, d, 0.2).astype(np.float32)
    X[7, 40] = 70000.0
    X[150, 3] = -70000.0
    y = _labels(rng, n)
    indptr, indices, data = _csr_arrays(X)
    s = R.Solver(n, d, "erm", reg=0.1, storage="fp16")
    with pytest.raises(ValueError) as dense:
        s.set_data(X, y)
    assert "fp16 storage: 2 finite entries do not fit float16" in str(dense.value)
    assert "first at row 7, column 40 (value 70000)" in str(dense.value)
    for dev in (False, True):
        for itype in IDX.values():
            X2 = X.copy()
            X2[7, 40] = X2[150, 3] = 1.0
            s.set_data(X2, y)
            with pytest.raises(ValueError) as e:
                s.set_data(_source(R, torch, X.shape, indptr, indices, data, itype, dev), y)
            assert str(e.value) == str(dense.value)
            assert _stepped(R, s) == R._lib.RBL_ERR_STATE     # the handle is left without data
    s.set_data(sp.csr_matrix(X2), y)
    assert _same(s.get_D(), scaling_ref.form_D(X2.astype(np.float64), y, None, None, "fp16"))
    s.close()


def test_a_device_tensor_with_unsorted_rows_is_refused_by_the_library(R, torch):
    crow = torch.tensor([0, 2, 4], dtype=torch.int64)
    col = torch.tensor([0, 2, 3, 1], dtype=torch.int64)   # row 1: 3 before 1
    T = torch.sparse_csr_tensor(crow, col, torch.tensor([1.0, 2.0, 3.0, 4.0]), size=(2, 4), check_invariants=False).cuda()
    s = R.Solver(2, 4, "erm", reg=0.1, storage="f32", objective_only=True)
    with pytest.raises(ValueError, match="row 1: column index 1 follows 3.*coalesce"):
        s.set_data(T, np.ones(2))
    s.close()


# ------------------------------------------------------------------------------------------------- whole objects
KW = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
ITERS = 25


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(21)
    n, d = 600, 37
    A = sp.random(n, d, density=0.1, format="csr", dtype=np.float64, random_state=rng)
    A.data = (A.data * 4.0 - 2.0).astype(np.float64)
    A = A.astype(np.float32)
    Xd = A.toarray()
    w = rng.standard_normal(d)
    y = np.where(Xd.astype(np.float64) @ w + 0.3 * rng.standard_normal(n) > 0, 1.0, -1.0)
    lab = rng.integers(0, 3, n)
    return A, Xd, y, lab


def _state(s):
    st = s._s.get_state()
    return st["w"], st["z"], st["lam"]


@pytest.mark.parametrize("storage", ["f64", "f32", "fp16"])
def test_admm_on_scipy_csr_with_standardize_and_intercept(R, problem, storage):
    A, Xd, y, _ = problem
    kw = dict(max_iter=ITERS, tol=0, storage=storage, standardize=True, fit_intercept=True, **KW)
    a, b = R.ADMMmethod(A, y, **kw), R.ADMMmethod(Xd, y, **kw)
    assert _same(a.scale_mean_, b.scale_mean_) and _same(a.scale_scale_, b.scale_scale_)
    assert _same(a._s.get_D(), b._s.get_D())
    a.start_store(A[:200], y[:200], **KW)                 # a sparse test matrix
    b.start_store(Xd[:200], y[:200], **KW)
    a.main_loop(verbose=False)
    b.main_loop(verbose=False)
    for u, v in zip(_state(a), _state(b)):
        assert _same(u, v)
    assert len(a.test_losses) == ITERS + 1 and a.test_losses == b.test_losses


def test_admm_on_a_device_sparse_csr_tensor(R, torch, problem):
    A, Xd, y, _ = problem
    T = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                torch.from_numpy(A.data), size=A.shape).cuda()
    src = R._solver.as_source(T, 0)
    assert src.mem == R._lib.MEM_DEVICE and src.values == T.values().data_ptr() and src.indptr == T.crow_indices().data_ptr()
    a = R.ADMMmethod(T, y, max_iter=ITERS, tol=0, storage="f32", **KW)
    b = R.ADMMmethod(Xd, y, max_iter=ITERS, tol=0, storage="f32", **KW)
    assert _same(a._s.get_D(), b._s.get_D())
    a.main_loop(verbose=False)
    b.main_loop(verbose=False)
    for u, v in zip(_state(a), _state(b)):
        assert _same(u, v)


def test_group_on_sparse_input(R, problem):
    A, Xd, y, _ = problem
    problems = [dict(weight_function="erm", l2_reg=0.01), dict(weight_function="superquantile", args=[0.5], l2_reg=0.01),
                dict(weight_function="aorr", args=[0.2, 0.8], l1_reg=0.01)]
    ga = R.ADMMgroup(A, y, problems, storage="f32", max_iter=ITERS, tol=0)
    gb = R.ADMMgroup(Xd, y, problems, storage="f32", max_iter=ITERS, tol=0)
    ga.start_store(A[:200], y[:200])
    gb.start_store(Xd[:200], y[:200])
    Wa, Wb = ga.main_loop(verbose=False), gb.main_loop(verbose=False)
    for sa, sb, wa, wb in zip(ga.solvers, gb.solvers, Wa, Wb):
        assert _same(wa, wb) and sa.test_losses == sb.test_losses
        for u, v in zip(_state(sa), _state(sb)):
            assert _same(u, v)
    ga.close()
    gb.close()


def test_one_vs_rest_and_accuracy_on_sparse_input(R, problem):
    A, Xd, y, lab = problem
    kw = dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.01, max_iter=ITERS, tol=0, storage="f32")
    a, b = R.OneVsRest(A, lab, **kw), R.OneVsRest(Xd, lab, **kw)
    Wa, Wb = a.main_loop(verbose=False), b.main_loop(verbose=False)
    assert Wa.shape == (37, 3) and _same(Wa, Wb)
    assert np.array_equal(a.predict(A[:250]), b.predict(Xd[:250]))
    assert a.accuracy(A[:250], lab[:250]) == b.accuracy(Xd[:250], lab[:250])
    a.close()
    b.close()
    from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
    w = Wa[:, 0]
    assert calculate_accuracy(w, A, y) == calculate_accuracy(w, Xd, y)
    assert calculate_accuracy(w, A.tocsc(), y, loss="squared_hinge") == calculate_accuracy(w, Xd, y, loss="squared_hinge")
