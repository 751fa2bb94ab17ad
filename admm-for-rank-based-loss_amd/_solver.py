"""Thin object wrapper over a librbl solver handle (include/rbl.h).  Host logic only:
argument checking with the reference's error messages, buffer marshalling, and the
per-phase calls.  Every number is computed by the HIP library."""
import ctypes as C
import math
import sys

import numpy as np

try:
    from . import _lib
except ImportError:  # package directory itself on sys.path (drop-in `src.optim` layout)
    import _lib

_FAMILIES = "['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']"
_LOSSES = "['binary_cross_entropy', 'multinomial_cross_entropy', 'hinge', 'squared_hinge']"


def check_problem(weight_function, loss, B, args, need_prox=True):
    """Argument validation in the order the reference performs it
    (rankbasedObjective.__init__ src/optim/objective.py:46-58, then
    Optimizer.__init__ src/optim/algorithms.py:64-68)."""
    if weight_function not in _lib.WEIGHT:
        if weight_function not in ("erm", "ehrm") and args is None:
            raise ValueError("args for framework is None!")                      # objective.py:171-172
        raise ValueError(f"Unrecognized framework '{weight_function}'! Options: {_FAMILIES}")  # :185-187
    if weight_function not in ("erm", "ehrm") and args is None:
        raise ValueError("args for framework is None!")
    if weight_function == "aorr_dc" and args[0] <= args[1]:
        raise ValueError("need args[0] > args[1]!")                              # objective.py:140-141
    if loss not in ("binary_cross_entropy", "multinomial_cross_entropy", "hinge", "squared_hinge"):
        raise ValueError(f"Unrecognized loss '{loss}'! Options: {_LOSSES}")      # objective.py:35-37
    if B is not None and loss != "binary_cross_entropy":
        raise ValueError("erhm only can be with the binary_cross_entropy.")      # objective.py:57-58
    if loss == "multinomial_cross_entropy" and need_prox:
        # the reference accepts it in the objective but its z-step has no prox for it
        # (src/util/individual_solver.py:124-125 is `pass`): unsupported there too
        raise ValueError(f"Unrecognized loss '{loss}'! Options: ['binary_cross_entropy', 'hinge', 'squared_hinge'] for the ADMM z-step")


def _as_labels(y, n):
    y = np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y)
    y = np.ascontiguousarray(y.reshape(-1), dtype=np.float64)
    if y.shape[0] != n:
        raise ValueError(f"y has {y.shape[0]} labels for {n} rows")
    if np.all((y == 0) | (y == 1)):     # objective.py:12 turns -1 into 0 in place; accept both
        y = 2.0 * y - 1.0
    return y


def as_pm1_labels(y, n, what="y"):
    """n labels in {+1, -1} ({0, 1} is accepted as in _as_labels); anything else is a ValueError naming `what`."""
    try:
        y = _as_labels(y, n)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    if not np.all((y == 1.0) | (y == -1.0)):
        bad = int(np.flatnonzero(~((y == 1.0) | (y == -1.0)))[0])
        raise ValueError(f"{what}: labels must be +1/-1 (entry {bad} is {y[bad]!r})")
    return y


def as_penalty(v, d, what):
    """A penalty vector: a scalar or d values, finite and >= 0 -> float64 (d,); anything else is a ValueError naming
    `what`.  Checked on the host, before any device call."""
    a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    try:
        a = np.asarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected a number or {d} numbers") from None
    if a.ndim == 0 or a.size == 1 and d != 1:
        a = np.full(d, float(a.reshape(-1)[0]) if a.size else np.nan)
    a = np.ascontiguousarray(a.reshape(-1))
    if a.shape[0] != d:
        raise ValueError(f"{what}: has {a.shape[0]} entries for {d} coordinates")
    if not np.all(np.isfinite(a)):
        bad = int(np.flatnonzero(~np.isfinite(a))[0])
        raise ValueError(f"{what}: entries must be finite (entry {bad} is {a[bad]!r})")
    if np.any(a < 0):
        bad = int(np.flatnonzero(a < 0)[0])
        raise ValueError(f"{what}: entries must be >= 0 (entry {bad} is {a[bad]!r})")
    return a


def resolve_penalty(d, l1_reg=None, l2_reg=None, l1_weights=None, l2_weights=None, fit_intercept=False):
    """Per-coordinate penalties of a problem with d features (include/rbl.h: rbl_set_penalty).

    None when none of l1_weights / l2_weights / fit_intercept is given: the scalar path, exactly as before.  Otherwise a
    dict: ``l1`` / ``l2`` (d values each, d + 1 with the intercept's zeros appended), ``wstep`` (the lasso form if any
    l1 > 0, else the ridge form) and ``reg`` (mean of the feature's l1 weights if any is positive, else of the l2
    weights) - it only sets the reference's starting values, so l1_weights=a starts where l1_reg=a does.  Each norm takes
    its weights if given, else its scalar; with no weights at all and both scalars given the reference's rule stays:
    l1_reg is used."""
    if l1_weights is None and l2_weights is None and not fit_intercept:
        return None
    if l1_weights is None and l2_weights is None and l1_reg is not None:
        l2_reg = None                                  # algorithms.py:30, :57-60: l1_reg wins
    l1 = as_penalty(l1_weights if l1_weights is not None else (0.0 if l1_reg is None else l1_reg), d,
                    "l1_weights" if l1_weights is not None else "l1_reg")
    l2 = as_penalty(l2_weights if l2_weights is not None else (0.0 if l2_reg is None else l2_reg), d,
                    "l2_weights" if l2_weights is not None else "l2_reg")
    if not (np.any(l1 > 0) or np.any(l2 > 0)):
        raise ValueError("More arguments: l1_reg, l2_reg, l1_weights or l2_weights must hold a positive penalty")
    any_l1 = bool(np.any(l1 > 0))
    v = l1 if any_l1 else l2
    reg = float(v[0]) if np.all(v == v[0]) else float(np.mean(v))     # (a constant vector: its value, not a rounded mean)
    if fit_intercept:
        l1, l2 = np.append(l1, 0.0), np.append(l2, 0.0)
    return dict(l1=l1, l2=l2, wstep=_lib.WSTEP_L1 if any_l1 else _lib.WSTEP_L2, reg=reg)


def as_row_weights(c, n, what="sample_weight"):
    """Row weights: n values, finite and >= 0, at least one > 0 -> float64 (n,); anything else is a ValueError naming
    `what` and the first offending row.  Checked on the host, before any device call."""
    a = np.asarray(c.detach().cpu().numpy() if hasattr(c, "detach") else c)
    try:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected {n} numbers") from None
    if a.shape[0] != n:
        raise ValueError(f"{what}: has {a.shape[0]} entries for {n} rows")
    if not np.all(np.isfinite(a)):
        bad = int(np.flatnonzero(~np.isfinite(a))[0])
        raise ValueError(f"{what}: weights must be finite (row {bad} is {a[bad]!r})")
    if np.any(a < 0):
        bad = int(np.flatnonzero(a < 0)[0])
        raise ValueError(f"{what}: weights must be >= 0 (row {bad} is {a[bad]!r})")
    if n > 0 and not np.any(a > 0):
        raise ValueError(f"{what}: all {n} weights are zero - at least one must be > 0")
    return a


def resolve_row_weights(y_pm1, sample_weight=None, class_weight=None, weight_function="erm"):
    """The row weights c of F(w) = (1/n) sum_i c_i loss_i(w) + R(w) (include/rbl.h: rbl_set_row_weights) from the two
    keywords, or None when neither is given (the unweighted path, exactly as before).

    class_weight: "balanced" gives c_i = n / (2 n_{y_i}); a dict {+1: a, -1: b} is taken as given.  sample_weight (n
    values) multiplies in.  No normalisation.  Everything is checked here, on the host, before any device call; a
    rank-weighted family is refused: with weights the sigma of a rank depends on the cumulative weight in sorted order,
    so it is not fixed per rank and the PAV z-step does not apply."""
    if sample_weight is None and class_weight is None:
        return None
    if weight_function != "erm":
        raise ValueError(f'sample_weight / class_weight need weight_function="erm" (got {weight_function!r}): with row '
                         "weights the sigma of a rank depends on the cumulative weight in sorted order, so it is not "
                         "fixed per rank and the PAV z-step does not apply")
    y = np.asarray(y_pm1, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    c = np.ones(n)
    if class_weight is not None:
        pos = y > 0
        if isinstance(class_weight, str):
            if class_weight != "balanced":
                raise ValueError(f'class_weight must be "balanced" or a dict {{+1: a, -1: b}} (got {class_weight!r})')
            n_pos, n_neg = int(np.count_nonzero(pos)), int(n - np.count_nonzero(pos))
            if n_pos == 0 or n_neg == 0:
                raise ValueError('class_weight="balanced": both classes must be present')
            a, b = n / (2.0 * n_pos), n / (2.0 * n_neg)
        elif isinstance(class_weight, dict):
            if set(class_weight) != {1, -1}:
                raise ValueError(f"class_weight: the dict must have exactly the keys +1 and -1 (got {sorted(class_weight, key=repr)})")
            a, b = float(class_weight[1]), float(class_weight[-1])
            for k, v in ((1, a), (-1, b)):
                if not np.isfinite(v) or v < 0:
                    raise ValueError(f"class_weight[{k:+d}] must be finite and >= 0 (got {v!r})")
        else:
            raise ValueError(f'class_weight must be "balanced" or a dict {{+1: a, -1: b}} (got {class_weight!r})')
        c = np.where(pos, a, b).astype(np.float64)
    if sample_weight is not None:
        c = c * as_row_weights(sample_weight, n)
    return as_row_weights(c, n, "sample_weight * class_weight" if class_weight is not None else "sample_weight")


def add_intercept_column(X):
    """[X | 1]: a host copy of X with a column of ones appended (fit_intercept=True)"""
    return np.ascontiguousarray(np.hstack([X, np.ones((X.shape[0], 1))]))


def _is_scipy_sparse(X):
    """a scipy.sparse matrix or array (SciPy is looked at only if the caller has imported it)"""
    sp = sys.modules.get("scipy.sparse")
    return sp is not None and sp.issparse(X)


def _is_torch_sparse(X):
    return hasattr(X, "detach") and hasattr(X, "layout") and "sparse" in str(X.layout)


def _as_matrix(X):
    """X as a C-contiguous float64 host array (the baselines' path, and what as_source falls back to); sparse input is
    densified - the baselines mirror the reference, which works on dense rows"""
    if _is_scipy_sparse(X):
        X = X.toarray()
    elif _is_torch_sparse(X):
        X = X.detach().to_dense()
    X = X.detach().cpu().numpy() if hasattr(X, "detach") else np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be a 2-D array")
    return np.ascontiguousarray(X, dtype=np.float64)


_SOURCE_TYPES = "float64, float32 and float16"


class Source:
    """A data matrix as rbl_set_data_from takes it: ``ptr`` (integer address), ``dtype`` (_lib.DTYPE_*), ``mem``
    (_lib.MEM_HOST / MEM_DEVICE), ``ldx`` (row stride in elements), ``shape`` and ``keep`` - the object that owns the
    memory (the caller's array or tensor itself when it is used in place)."""
    __slots__ = ("ptr", "dtype", "mem", "ldx", "shape", "keep")

    def __init__(self, ptr, dtype, mem, ldx, shape, keep):
        self.ptr, self.dtype, self.mem, self.ldx, self.shape, self.keep = int(ptr), dtype, mem, int(ldx), tuple(shape), keep


class CsrSource:
    """A sparse data matrix as rbl_set_data_csr takes it: ``shape``, ``dtype`` (_lib.DTYPE_* of the values), ``mem``
    (_lib.MEM_HOST / MEM_DEVICE, of all three arrays), ``index_type`` (_lib.INDEX_*, of indptr and indices), ``nnz``,
    the integer addresses ``indptr`` / ``indices`` / ``values`` and ``keep`` - the objects that own the memory (the
    caller's own arrays when they are used in place)."""
    __slots__ = ("shape", "dtype", "mem", "index_type", "nnz", "indptr", "indices", "values", "keep")

    def __init__(self, shape, dtype, mem, index_type, nnz, indptr, indices, values, keep):
        self.shape, self.dtype, self.mem, self.index_type, self.nnz = tuple(int(v) for v in shape), dtype, mem, index_type, int(nnz)
        self.indptr, self.indices, self.values, self.keep = int(indptr), int(indices), int(values), keep


def _host_array(a, dtype):
    """a as a native, aligned, C-contiguous 1-D array of dtype - a itself when it already is one"""
    if isinstance(a, np.ndarray) and a.dtype == dtype and a.dtype.isnative and a.ndim == 1 and a.flags["C_CONTIGUOUS"] \
            and a.flags["ALIGNED"]:
        return a
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _csr_from_scipy(X):
    """SciPy sparse -> CsrSource.  A canonical csr_matrix / csr_array with float64 / float32 data is used in place; other
    formats go through tocsr(), a non-canonical matrix is copied and sum_duplicates() runs on the copy (the caller's
    object is never modified); integer / bool data become float64; indptr and indices of different widths, or of a type
    other than int32 / int64, become int64."""
    A = X
    if A.ndim != 2:
        raise ValueError("X must be a 2-D array")
    if A.dtype.kind == "c":
        raise ValueError(f"X has dtype {A.dtype}: the supported element types are {_SOURCE_TYPES}")
    if A.format != "csr":
        A = A.tocsr()
    if not A.has_canonical_format:
        if A is X:
            A = A.copy()
        A.sum_duplicates()
    vt = A.data.dtype if A.data.dtype in (np.dtype(np.float64), np.dtype(np.float32)) else np.dtype(np.float64)
    it = A.indptr.dtype if A.indptr.dtype == A.indices.dtype and A.indptr.dtype in _lib.INDEX_DTYPE else np.dtype(np.int64)
    indptr, indices, data = _host_array(A.indptr, it), _host_array(A.indices, it), _host_array(A.data, vt)
    return CsrSource(A.shape, _lib.SOURCE_DTYPE[vt], _lib.MEM_HOST, _lib.INDEX_DTYPE[it], data.shape[0], indptr.ctypes.data,
                     indices.ctypes.data, data.ctypes.data, (A, indptr, indices, data))


def _csr_from_torch(X, device):
    """torch sparse tensor -> CsrSource.  A sparse_csr tensor with float64 / float32 / float16 values is used in place, on
    the CPU or on the solver's GPU (its current stream is synchronised first); COO and CSC go through to_sparse_csr();
    integer / bool values become float64.  bfloat16, complex, batched or hybrid tensors and tensors on another device are
    a ValueError.  The rows of a device tensor are checked by the library (canonical CSR)."""
    import torch
    t = X.detach()
    if t.dim() != 2 or t.dense_dim() != 0:
        raise ValueError("X must be a 2-D array (a batched or hybrid sparse tensor has no instance)")
    kinds = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16}
    if t.dtype not in kinds and (t.dtype.is_floating_point or t.dtype.is_complex):
        raise ValueError(f"X has dtype {t.dtype}: the supported element types are {_SOURCE_TYPES}")
    if t.device.type not in ("cpu", "cuda"):
        raise ValueError(f"X lives on {t.device}: host memory or the solver's GPU (element types {_SOURCE_TYPES})")
    if t.device.type == "cuda" and device is not None and t.device.index != int(device):
        raise ValueError(f"X lives on {t.device}, the solver on device {int(device)}: move it there (supported "
                         f"element types: {_SOURCE_TYPES})")
    if t.layout != torch.sparse_csr:
        if t.layout == torch.sparse_coo:
            t = t.coalesce()
        t = t.to_sparse_csr()
    if t.dtype not in kinds:
        t = t.to(torch.float64)
    crow, col, val = t.crow_indices(), t.col_indices(), t.values()
    if crow.dtype != col.dtype or crow.dtype not in (torch.int32, torch.int64):
        crow, col = crow.to(torch.int64), col.to(torch.int64)
    crow, col, val = crow.contiguous(), col.contiguous(), val.contiguous()
    if t.device.type == "cuda":
        torch.cuda.current_stream(t.device).synchronize()          # X's writes are complete before the library reads it
    return CsrSource(t.shape, kinds[t.dtype], _lib.MEM_DEVICE if t.device.type == "cuda" else _lib.MEM_HOST,
                     _lib.INDEX_I32 if crow.dtype == torch.int32 else _lib.INDEX_I64, val.shape[0], crow.data_ptr(),
                     col.data_ptr(), val.data_ptr(), (t, crow, col, val))


def _row_stride(shape, strides, itemsize):
    """row stride in elements if the rows are contiguous and the stride a positive multiple of the item size, else None"""
    n, d = shape
    if n == 0 or d == 0:
        return None
    if d > 1 and strides[1] != itemsize:
        return None
    if n == 1:
        return d
    if strides[0] <= 0 or strides[0] % itemsize or strides[0] < d * itemsize:
        return None
    return strides[0] // itemsize


def as_source(X, device=None):
    """X in the type it has and from where it lives (include/rbl.h: rbl_set_data_from) -> Source; a scipy.sparse
    matrix / array or a torch sparse tensor -> CsrSource (rbl_set_data_csr: _csr_from_scipy, _csr_from_torch).

    No copy for NumPy float64 / float32 / float16 arrays with contiguous rows (a column slice of a wider array is used
    in place with its row stride), for torch CPU tensors of those types (a view) and for torch tensors on the handle's
    GPU (``device``: its index; the tensor's current stream is synchronised first).  A tensor on the GPU whose rows are
    not contiguous (transposed, strided columns) stays there: ``contiguous()`` makes a second copy of it ON THE DEVICE,
    in its own type, for the duration of the call - for a tensor of tens of GB pass contiguous rows.  Integer / bool data, Fortran
    order, negative strides and lists are converted to a C-contiguous float64 host array.  A tensor on another device,
    or of a type the library has no instance for (bfloat16, complex), is a ValueError."""
    if isinstance(X, (Source, CsrSource)):
        return X
    if _is_scipy_sparse(X):
        return _csr_from_scipy(X)
    if _is_torch_sparse(X):
        return _csr_from_torch(X, device)
    if hasattr(X, "detach") and hasattr(X, "data_ptr"):
        import torch
        t = X.detach()
        if t.dim() != 2:
            raise ValueError("X must be a 2-D array")
        kinds = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16}
        if t.dtype not in kinds and (t.dtype.is_floating_point or t.dtype.is_complex):
            raise ValueError(f"X has dtype {t.dtype}: the supported element types are {_SOURCE_TYPES}")
        if t.device.type == "cuda" and t.dtype in kinds:
            if device is not None and t.device.index != int(device):
                raise ValueError(f"X lives on {t.device}, the solver on device {int(device)}: move it there (supported "
                                 f"element types: {_SOURCE_TYPES})")
            ldx = _row_stride(tuple(t.shape), tuple(st * t.element_size() for st in t.stride()), t.element_size())
            if ldx is None:
                t = t.contiguous()          # (a copy on the device: transposed or strided columns)
                ldx = t.shape[1]
            torch.cuda.current_stream(t.device).synchronize()      # X's writes are complete before the library reads it
            return Source(t.data_ptr(), kinds[t.dtype], _lib.MEM_DEVICE, ldx, t.shape, t)
        if t.device.type not in ("cpu", "cuda"):
            raise ValueError(f"X lives on {t.device}: host memory or the solver's GPU (element types {_SOURCE_TYPES})")
        X = t.cpu().numpy()                 # a view of a CPU tensor; integer / bool tensors are converted below
    A = X if isinstance(X, np.ndarray) else np.asarray(X)
    if A.ndim != 2:
        raise ValueError("X must be a 2-D array")
    if A.dtype.kind == "c":
        raise ValueError(f"X has dtype {A.dtype}: the supported element types are {_SOURCE_TYPES}")
    dt = _lib.SOURCE_DTYPE.get(A.dtype) if A.dtype.isnative else None
    ldx = _row_stride(A.shape, A.strides, A.itemsize) if dt is not None and A.flags["ALIGNED"] else None
    if ldx is None:
        A = np.ascontiguousarray(A, dtype=np.float64)
        dt, ldx = _lib.DTYPE_F64, max(A.shape[1], 1)
    return Source(A.ctypes.data, dt, _lib.MEM_HOST, ldx, A.shape, A)


def resolve_standardize(standardize):
    """The ``standardize`` keyword -> False, True (centre and scale) or "scale" (unit-variance columns without centring:
    the mean vector is all zeros, a sparse X stays sparse).  Any other string is a ValueError."""
    if isinstance(standardize, str):
        if standardize != "scale":
            raise ValueError(f'standardize must be False, True or "scale", got {standardize!r}')
        return "scale"
    return bool(standardize)


def check_csr_storage(src, storage, standardize=False, what="X"):
    """storage="csr" keeps D sparse: it takes a sparse matrix as it is and no centring (it makes the columns dense);
    standardize="scale" scales without it.  Raises ValueError - before any device call - for a dense ``src`` (a Source)
    or standardize=True."""
    if storage != "csr":
        return
    if standardize and standardize != "scale":
        raise ValueError('standardize=True with storage="csr": centring the columns makes D dense - scale the sparse '
                         "matrix yourself (scaling without centring keeps it sparse) or use a dense storage type; "
                         'standardize="scale" does that scaling on the device')
    if not isinstance(src, CsrSource):
        raise ValueError(f'storage="csr" needs a sparse {what} (scipy.sparse matrix / array or torch sparse tensor); '
                         f"this one is dense - pass scipy.sparse.csr_matrix({what}), or use storage f32 / f64 / fp16")


def resolve_gram(gram, storage, d):
    """The w-step route of a problem with d coordinates: "dense" (Gram space: G = D^T D is formed) or "none" (the
    operator w-step of RBL_CREATE_NO_GRAM: no d x d matrix).  ``gram="auto"`` is "none" exactly where the Gram route
    cannot run - storage "csr" with ld > 16 384 - and "dense" everywhere else.  "none" needs storage "csr"; "dense" on
    "csr" needs ld <= 16 384.  Raises ValueError - before any device call - otherwise."""
    if gram not in _lib.GRAM_MODES:
        raise ValueError(f"gram must be one of {list(_lib.GRAM_MODES)}, got {gram!r}")
    if storage not in _lib.STORAGE:
        raise ValueError(f"storage must be one of {sorted(_lib.STORAGE)}")
    wide = storage == "csr" and _lib.storage_ld(d, storage) > _lib.GRAM_MAX_LD
    if gram == "auto":
        return "none" if wide else "dense"
    if gram == "none" and storage != "csr":
        raise ValueError(f'gram="none" needs storage="csr" (the operator w-step runs on the sparse passes), got storage={storage!r}')
    if gram == "dense" and wide:
        raise ValueError(f'gram="dense" with storage="csr" and {d} coordinates: the Gram-space w-step stops at '
                         f'{_lib.GRAM_MAX_LD} - use gram="none" (or "auto")')
    return gram


def resolve_l1_solver(l1_solver, has_l1, storage, gram_route):
    """The l1 w-step of a gram="none" solver: "fista" (FISTA on the operator - the default, and the only value elsewhere)
    or "working_set" (the exact working-set lasso, RBL_CREATE_WORKING_SET).  "working_set" needs an l1 penalty
    (l1_reg / l1_weights), storage "csr" and the gram="none" route.  Raises ValueError - before any device call -
    otherwise.  -> the create flag it adds (0 for "fista")."""
    check_l1_solver(l1_solver)
    if l1_solver == "fista":
        return 0
    if not has_l1:
        raise ValueError('l1_solver="working_set" is the lasso / elastic-net w-step: it needs l1_reg or l1_weights')
    if storage != "csr":
        raise ValueError(f'l1_solver="working_set" needs storage="csr" (the working set is built from the sparse entries), '
                         f"got storage={storage!r}")
    if gram_route != "none":
        raise ValueError('l1_solver="working_set" needs gram="none": with gram="dense" the l1 w-step is the exact active-set '
                         "kernel on G already")
    return _lib.CREATE_WORKING_SET


def as_scaling(mean, scale, d, ones_column=False):
    """(mean, scale) for d coordinates as float64; with ones_column the vectors of the d - 1 features are accepted and
    the unscaled column's (0, 1) appended"""
    mean, scale = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (mean, scale))
    if ones_column and mean.size == d - 1 and scale.size == d - 1:
        mean, scale = np.append(mean, 0.0), np.append(scale, 1.0)
    if mean.size != d or scale.size != d:
        raise ValueError(f"scaling: mean / scale have {mean.size} / {scale.size} entries for {d} columns")
    return mean, scale


class Solver:
    """One librbl handle.  ``n`` local rows of an ``n_total``-row problem.  ``share``: another Solver whose device D and
    Gram matrix this one borrows (include/rbl.h: rbl_create_shared) - no set_data / gram on this handle.  ``gram``: the
    w-step's route (resolve_gram; ``gram_route`` holds "dense" or "none" - "none" creates the handle with
    RBL_CREATE_NO_GRAM); with ``share`` it must be the owner's."""

    def __init__(self, n, d, weight_function="erm", loss="binary_cross_entropy", reg=0.0, wstep=_lib.WSTEP_L2,
                 B=None, args=None, smooth_t=1.0, rho0=0.0, tol=1e-4, w_tol=0.0, max_iter=200, storage="f32",
                 device=0, objective_only=False, n_total=None, row_offset=0, share=None, gram="auto", l1_solver="fista"):
        self._h = None
        self._center = True           # what set_centering last set (the library's default)
        self._share = share           # keeps the data's owner referenced (the library counts references itself)
        if storage not in _lib.STORAGE:
            raise ValueError(f"storage must be one of {sorted(_lib.STORAGE)}")
        # "dense" or "none" (resolve_gram); a borrower is what its owner is - asking it for the other route is an error
        self.gram_route = resolve_gram(gram, storage, d)
        if not objective_only and self.gram_route == "none" and int(wstep) == _lib.WSTEP_SMOOTH_L1:
            raise ValueError('the smoothed-l1 w-step needs the Gram matrix (its preconditioner is diag(G)): it has no '
                             'gram="none" route' + (f" - and storage=\"csr\" with {d} coordinates has no other" if gram == "auto" else ""))
        if isinstance(share, Solver) and not objective_only and not share.cfg.objective_only and share.gram_route != self.gram_route:
            raise ValueError(f'gram={gram!r} on data shared with a gram="{share.gram_route}" solver: one data matrix, one route')
        # "fista" or "working_set" (resolve_l1_solver); a borrower is what its owner is
        ws_flag = 0 if objective_only else resolve_l1_solver(l1_solver, int(wstep) == _lib.WSTEP_L1, storage, self.gram_route)
        self.l1_solver = "working_set" if ws_flag else "fista"
        if isinstance(share, Solver) and not objective_only and not share.cfg.objective_only and \
                getattr(share, "l1_solver", "fista") != self.l1_solver:
            raise ValueError(f'l1_solver={l1_solver!r} on data shared with an l1_solver="{getattr(share, "l1_solver", "fista")}" '
                             "solver: a borrower follows its owner")
        self.lib = _lib.load()
        cfg = _lib.RblConfig()
        cfg.n, cfg.d = int(n), int(d)
        cfg.n_total = int(n if n_total is None else n_total)
        cfg.row_offset = int(row_offset)
        cfg.loss = _lib.LOSS[loss]
        cfg.weight_function = _lib.WEIGHT[weight_function]
        a = list(args) if args is not None else []
        cfg.n_weight_args = min(len(a), 2)
        for k in range(cfg.n_weight_args):
            cfg.weight_args[k] = float(a[k])
        cfg.has_B = 0 if B is None else 1
        cfg.B = 0.0 if B is None else float(B)
        cfg.wstep = int(wstep)
        cfg.reg = float(reg)
        cfg.smooth_t = float(smooth_t)
        cfg.rho0 = float(rho0)
        cfg.tol = float(tol)
        cfg.w_tol = float(w_tol)
        cfg.max_iter = int(max_iter)
        cfg.storage = _lib.STORAGE[storage]
        cfg.device = int(device)
        cfg.objective_only = 1 if objective_only else 0
        self.cfg = cfg
        self.n, self.d, self.n_total = cfg.n, cfg.d, cfg.n_total
        h = C.c_void_p()
        if share is not None:
            if not isinstance(share, Solver) or not share._h:
                raise ValueError("share must be a live Solver")
            _lib.check(self.lib.rbl_create_shared(C.byref(cfg), share._h, C.byref(h)))
        else:
            flags = (_lib.CREATE_NO_GRAM if self.gram_route == "none" and not objective_only else 0) | ws_flag
            _lib.check(self.lib.rbl_create_opts(C.byref(cfg), flags, C.byref(h)))
        self._h = h

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None):
            self.lib.rbl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------------- data
    def set_data(self, X, y, scaling="none", ones_column=False):
        """D = -y * X from X as it is (as_source: float64 / float32 / float16, host or this handle's GPU; include/rbl.h:
        rbl_set_data_from; sparse X: CSR arrays expanded on the device, rbl_set_data_csr).  scaling: "none", "fit" (standardise the columns on the device, keep the vectors:
        get_scaling) or "apply" (the vectors of set_scaling).  ones_column: X has d - 1 columns, column d - 1 of D is
        -y * 1 (the intercept's), never scaled.  Labels are a host float64 vector (a device y is copied, 8 bytes a row)."""
        if scaling not in _lib.SCALING:
            raise ValueError(f"scaling must be one of {sorted(_lib.SCALING)}")
        src = as_source(X, self.cfg.device)
        if self.cfg.storage == _lib.STORE_CSR:      # (scaling is allowed once centring is off: set_centering)
            check_csr_storage(src, "csr", scaling != "none" and self._center)
        y = _as_labels(y, src.shape[0])
        shape = (src.shape[0], src.shape[1] + (1 if ones_column else 0))
        if shape != (self.n, self.d):
            raise ValueError(f"X is {shape}, expected {(self.n, self.d)}")
        flags = _lib.DATA_ONES_COLUMN if ones_column else 0
        if isinstance(src, CsrSource):      # expanded on the device (include/rbl.h: rbl_set_data_csr)
            _lib.check(self.lib.rbl_set_data_csr(self._h, C.c_void_p(src.indptr), C.c_void_p(src.indices),
                                                 C.c_void_p(src.values), src.nnz, src.index_type, src.dtype, src.mem,
                                                 _lib.ptr(y), _lib.SCALING[scaling], flags))
            return
        _lib.check(self.lib.rbl_set_data_from(self._h, C.c_void_p(src.ptr), src.dtype, src.mem, src.ldx, _lib.ptr(y),
                                              _lib.SCALING[scaling], flags))

    def set_data_f64(self, X, y):
        """the float64 host route (include/rbl.h: rbl_set_data): X is converted to a C-contiguous float64 host array"""
        if self.cfg.storage == _lib.STORE_CSR:
            raise ValueError('storage="csr" takes its data through set_data (a sparse X); set_data_f64 uploads a dense matrix')
        X = _as_matrix(X)
        y = _as_labels(y, X.shape[0])
        if X.shape != (self.n, self.d):
            raise ValueError(f"X is {X.shape}, expected {(self.n, self.d)}")
        _lib.check(self.lib.rbl_set_data(self._h, _lib.ptr(X), _lib.ptr(y), X.shape[1]))

    def set_scaling(self, mean, scale):
        """the column means / scales scaling="apply" uses (d values each; None, None clears them)"""
        if mean is None and scale is None:
            _lib.check(self.lib.rbl_set_scaling(self._h, None, None))
            return
        mean, scale = as_scaling(mean, scale, self.d)
        _lib.check(self.lib.rbl_set_scaling(self._h, _lib.ptr(mean), _lib.ptr(scale)))

    def set_centering(self, center):
        """False: scaling="fit" / "apply" of the next set_data scale the columns without centring them (the mean vector is
        all zeros; include/rbl.h: rbl_set_centering) - the scaling a storage="csr" handle takes.  True: the default."""
        _lib.check(self.lib.rbl_set_centering(self._h, 1 if center else 0))
        self._center = bool(center)

    def get_centering(self):
        flag = C.c_int(1)
        _lib.check(self.lib.rbl_get_centering(self._h, C.byref(flag)))
        return bool(flag.value)

    def get_scaling(self):
        """(mean, scale) of scaling="fit" / set_scaling, or None when the handle has none"""
        mean, scale, flag = np.empty(self.d), np.empty(self.d), C.c_int(0)
        _lib.check(self.lib.rbl_get_scaling(self._h, _lib.ptr(mean), _lib.ptr(scale), C.byref(flag)))
        return (mean, scale) if flag.value else None

    def generate_synthetic(self, seed=17, class_sep=1.0, flip_y=0.01):
        _lib.check(self.lib.rbl_generate_synthetic(self._h, int(seed), float(class_sep), float(flip_y)))

    def synth_local(self, seed=17, class_sep=1.0, flip_y=0.01):
        _lib.check(self.lib.rbl_synth_local(self._h, int(seed), float(class_sep), float(flip_y)))

    def synth_finish(self):
        _lib.check(self.lib.rbl_synth_finish(self._h))

    def labels(self):
        y = np.empty(self.n)
        _lib.check(self.lib.rbl_get_labels(self._h, _lib.ptr(y)))
        return y

    def set_labels(self, y):
        """Labels of this handle's own on the data it borrows (include/rbl.h: rbl_set_labels): n values +-1, before the
        first iteration.  The shape and the values are checked here, before any device call."""
        y = as_pm1_labels(y, self.n)
        _lib.check(self.lib.rbl_set_labels(self._h, _lib.ptr(y)))

    def set_penalty(self, l1=None, l2=None):
        """Per-coordinate penalties R(w) = 1/2 sum_j (l1_j |w_j| + l2_j w_j^2) (include/rbl.h: rbl_set_penalty): a
        scalar or d values each, before the first iteration.  Shape, finiteness and sign are checked here first."""
        l1 = None if l1 is None else as_penalty(l1, self.d, "l1_weights")
        l2 = None if l2 is None else as_penalty(l2, self.d, "l2_weights")
        _lib.check(self.lib.rbl_set_penalty(self._h, _lib.ptr(l1), _lib.ptr(l2)))

    def get_penalty(self):
        """(l1, l2) of set_penalty, or None when the handle runs on its scalar reg"""
        l1, l2, flag = np.empty(self.d), np.empty(self.d), C.c_int(0)
        _lib.check(self.lib.rbl_get_penalty(self._h, _lib.ptr(l1), _lib.ptr(l2), C.byref(flag)))
        return (l1, l2) if flag.value else None

    def set_row_weights(self, c):
        """Row weights of an erm problem (include/rbl.h: rbl_set_row_weights): n values >= 0, at least one > 0, or None
        for the unweighted path.  Allowed between iterations.  Shape, finiteness and sign are checked here first."""
        if c is None:
            _lib.check(self.lib.rbl_set_row_weights(self._h, None))
            return
        c = as_row_weights(c, self.n)
        _lib.check(self.lib.rbl_set_row_weights(self._h, _lib.ptr(c)))

    def get_row_weights(self):
        """the weights of set_row_weights, or None when the handle has none"""
        c, flag = np.empty(self.n), C.c_int(0)
        _lib.check(self.lib.rbl_get_row_weights(self._h, _lib.ptr(c), C.byref(flag)))
        return c if flag.value else None

    def decide_multi(self, W):
        """argmax_j x_i . w_j over the rows of this handle's data (ties: lowest j); W: (k, d) -> int32 (n,)
        (include/rbl.h: rbl_decide_multi)"""
        W = _lib.f64(W)
        if W.ndim != 2 or W.shape[1] != self.d or not 1 <= W.shape[0] <= 64:
            raise ValueError(f"W must be (k, {self.d}) with 1 <= k <= 64, got {W.shape}")
        cls = np.empty(self.n, dtype=np.int32)
        _lib.check(self.lib.rbl_decide_multi(self._h, W.shape[0], _lib.ptr(W), _lib.ptr(cls)))
        return cls

    def gram(self):
        _lib.check(self.lib.rbl_gram_local(self._h))
        _lib.check(self.lib.rbl_gram_finish(self._h))

    def gram_local(self):
        _lib.check(self.lib.rbl_gram_local(self._h))

    def gram_finish(self):
        _lib.check(self.lib.rbl_gram_finish(self._h))

    def gram_info(self):
        """how the handle's last Gram matrix was formed (include/rbl.h: rbl_gram_report; a borrower: its owner's):
        route 0 none yet - or none at all (gram="none": the operator w-step) -, 1 dense storage, 2 csr by dense
        expansion, 3 csr from the entries"""
        rep = _lib.RblGramReport()
        _lib.check(self.lib.rbl_gram_info(self._h, C.byref(rep)))
        return _lib._gram_report_dict(rep)

    def wset_info(self):
        """the working set after the last w-step (include/rbl.h: rbl_wset_report) of an l1_solver="working_set" solver"""
        rep = _lib.RblWsetReport()
        _lib.check(self.lib.rbl_wset_info(self._h, C.byref(rep)))
        return _lib._wset_report_dict(rep)

    def get_D(self):
        out = np.empty((self.n, self.d))
        _lib.check(self.lib.rbl_get_D(self._h, _lib.ptr(out)))
        return out

    def set_stream(self, stream_ptr):
        """hipStream_t as an integer (0 = the default stream); None = the handle's own stream."""
        p = C.c_void_p(-1) if stream_ptr is None else C.c_void_p(int(stream_ptr))
        _lib.check(self.lib.rbl_set_stream(self._h, p))

    # --------------------------------------------------------------------- state
    def get_state(self, want_z=True, want_lam=True):
        w = np.empty(self.d)
        z = np.empty(self.n) if want_z and not self.cfg.objective_only else None
        lam = np.empty(self.n) if want_lam and not self.cfg.objective_only else None
        rho, it, t = C.c_double(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.rbl_get_state(self._h, _lib.ptr(w), _lib.ptr(z), _lib.ptr(lam), C.byref(rho),
                                          C.byref(it), C.byref(t)))
        return dict(w=w, z=z, lam=lam, rho=rho.value, iter=it.value, smooth_t=t.value)

    def set_state(self, w=None, z=None, lam=None, rho=None, iter=None, smooth_t=None):
        w = _lib.f64(w).reshape(-1) if w is not None else None
        z = _lib.f64(z).reshape(-1) if z is not None else None
        lam = _lib.f64(lam).reshape(-1) if lam is not None else None
        for a, k, name in ((w, self.d, "w"), (z, self.n, "z"), (lam, self.n, "lam")):
            if a is not None and a.size != k:
                raise ValueError(f"{name} has {a.size} entries, expected {k}")
        r = C.byref(C.c_double(rho)) if rho is not None else None
        i = C.byref(C.c_int64(iter)) if iter is not None else None
        t = C.byref(C.c_double(smooth_t)) if smooth_t is not None else None
        _lib.check(self.lib.rbl_set_state(self._h, _lib.ptr(w), _lib.ptr(z), _lib.ptr(lam), r, i, t))

    def sigma(self):
        a, b = np.empty(self.n_total), np.empty(self.n_total)
        _lib.check(self.lib.rbl_get_sigma(self._h, _lib.ptr(a), _lib.ptr(b)))
        return a, b

    def info(self):
        ld, cu, L = C.c_int64(0), C.c_int(0), C.c_double(0)
        _lib.check(self.lib.rbl_info(self._h, C.byref(ld), C.byref(cu), C.byref(L)))
        return dict(ld=ld.value, num_cu=cu.value, lipschitz=L.value)

    # ------------------------------------------------------------------ hot path
    def step(self, want_objective=False):
        st = _lib.RblStats()
        _lib.check(self.lib.rbl_step(self._h, 1 if want_objective else 0, C.byref(st)))
        return st

    def solve(self, max_iter=0, want_objective=False):
        cap = int(max_iter if max_iter > 0 else self.cfg.max_iter)
        hist = {k: np.full(cap, np.nan) for k in ("objective", "primal", "dual", "rho", "time")}
        st = _lib.RblStats()
        _lib.check(self.lib.rbl_solve(self._h, cap, 1 if want_objective else 0, C.byref(st),
                                      _lib.ptr(hist["objective"]), _lib.ptr(hist["primal"]), _lib.ptr(hist["dual"]),
                                      _lib.ptr(hist["rho"]), _lib.ptr(hist["time"]), cap))
        k = int(st.iter)
        return st, {name: a[:k] for name, a in hist.items()}

    def finalize_smooth(self):
        _lib.check(self.lib.rbl_finalize_smooth(self._h))

    def risk(self, w):
        """sum_i sigma_i loss_(i)(w) without the regulariser (objective.py:73-82)."""
        w = _lib.f64(w).reshape(-1)
        if w.size != self.d:
            raise ValueError(f"w has {w.size} entries, expected {self.d}")
        out = C.c_double(0)
        _lib.check(self.lib.rbl_objective(self._h, _lib.ptr(w), 0, C.byref(out)))
        return out.value

    def objective(self, w):
        """risk(w) + the handle's regulariser (cfg.reg, or the vectors of set_penalty)"""
        w = _lib.f64(w).reshape(-1)
        if w.size != self.d:
            raise ValueError(f"w has {w.size} entries, expected {self.d}")
        out = C.c_double(0)
        _lib.check(self.lib.rbl_objective(self._h, _lib.ptr(w), 1, C.byref(out)))
        return out.value

    def accuracy(self, w, threshold=0.5):
        """calculate_accuracy of src/util/calculate_acc.py:3-19 on this handle's rows."""
        w = _lib.f64(w).reshape(-1)
        if w.size != self.d:
            raise ValueError(f"w has {w.size} entries, expected {self.d}")
        out = C.c_double(0)
        _lib.check(self.lib.rbl_accuracy(self._h, _lib.ptr(w), float(threshold), C.byref(out)))
        return out.value

    def fair_statistics(self, w, group, threshold=0.5):
        """(SPD, DI, EOD, AOD, TI, FNRD) of src/util/fair_metric.py:3-41 on this handle's rows."""
        w = _lib.f64(w).reshape(-1)
        g = _lib.f64(group).reshape(-1)
        if w.size != self.d or g.size != self.n:
            raise ValueError("fair_statistics: w / group have the wrong size")
        out = np.empty(6)
        _lib.check(self.lib.rbl_fair_statistics(self._h, _lib.ptr(w), _lib.ptr(g), float(threshold), _lib.ptr(out)))
        return tuple(float(x) for x in out)

    # ---------------------------------------------------------------- phase API
    def phase_m(self):
        _lib.check(self.lib.rbl_phase_m(self._h))

    def phase_z(self, m_all_ptr=None):
        _lib.check(self.lib.rbl_phase_z(self._h, C.c_void_p(m_all_ptr) if m_all_ptr else None))

    def phase_z_external(self, z):
        """a z-step computed by the caller (overridden hook): n values for this handle's rows"""
        z = _lib.f64(z).reshape(-1)
        if z.size != self.n:
            raise ValueError(f"z has {z.size} entries, expected {self.n}")
        _lib.check(self.lib.rbl_phase_z_external(self._h, _lib.ptr(z)))

    def phase_w_external(self, w):
        """a w-step computed by the caller (overridden hook): d values"""
        w = _lib.f64(w).reshape(-1)
        if w.size != self.d:
            raise ValueError(f"w has {w.size} entries, expected {self.d}")
        _lib.check(self.lib.rbl_phase_w_external(self._h, _lib.ptr(w)))

    def phase_q(self):
        _lib.check(self.lib.rbl_phase_q(self._h))

    def phase_w(self):
        _lib.check(self.lib.rbl_phase_w(self._h))

    def phase_dual(self, want_objective=False):
        _lib.check(self.lib.rbl_phase_dual(self._h, 1 if want_objective else 0))

    def phase_finish(self):
        st = _lib.RblStats()
        _lib.check(self.lib.rbl_phase_finish(self._h, C.byref(st)))
        return st

    def buffer(self, which):
        p, cnt = C.c_void_p(), C.c_int64(0)
        _lib.check(self.lib.rbl_buffer(self._h, int(which), C.byref(p), C.byref(cnt)))
        return p.value, cnt.value

    # ---- distributed z-step (include/rbl.h: rbl_zd_*; driver: dist.py:_z_distributed)
    def zd_sort_local(self, nsamples):
        _lib.check(self.lib.rbl_zd_sort_local(self._h, int(nsamples)))

    def zd_partition(self, splitters_ptr, nparts, to_host=False):
        """counts per destination stay on the device (BUF_ZD_COUNTS); to_host=True also downloads them"""
        out = (C.c_int64 * int(nparts))() if to_host else None
        _lib.check(self.lib.rbl_zd_partition(self._h, C.c_void_p(splitters_ptr), int(nparts), out))
        return [int(x) for x in out] if to_host else None

    def zd_sort_losses(self, nsamples):
        _lib.check(self.lib.rbl_zd_sort_losses(self._h, int(nsamples)))

    def zd_risk(self, n_recv, sigma_off):
        _lib.check(self.lib.rbl_zd_risk(self._h, int(n_recv), int(sigma_off)))

    def zd_prepare(self, n_recv, sigma_off):
        _lib.check(self.lib.rbl_zd_prepare(self._h, int(n_recv), int(sigma_off)))

    def zd_pav(self, fvals_ptr):
        _lib.check(self.lib.rbl_zd_pav(self._h, C.c_void_p(fvals_ptr)))

    def zd_bounds(self):
        _lib.check(self.lib.rbl_zd_bounds(self._h))

    def zd_seam_setup(self, rank, world, level, bounds_all_ptr):
        _lib.check(self.lib.rbl_zd_seam_setup(self._h, int(rank), int(world), int(level), C.c_void_p(bounds_all_ptr)))

    def zd_seam_propose(self, K, cand_prev_ptr, part_prev_ptr):
        _lib.check(self.lib.rbl_zd_seam_propose(self._h, int(K), C.c_void_p(cand_prev_ptr), C.c_void_p(part_prev_ptr)))

    def zd_seam_eval(self, K, cand_all_ptr):
        _lib.check(self.lib.rbl_zd_seam_eval(self._h, int(K), C.c_void_p(cand_all_ptr)))

    def zd_seam_sums(self, K, cand_prev_ptr, part_prev_ptr, nseams):
        _lib.check(self.lib.rbl_zd_seam_sums(self._h, int(K), C.c_void_p(cand_prev_ptr), C.c_void_p(part_prev_ptr),
                                             int(nseams)))

    def zd_seam_fill(self, sums_ptr):
        _lib.check(self.lib.rbl_zd_seam_fill(self._h, C.c_void_p(sums_ptr)))

    def zd_return_partition(self, nmax, world, to_host=False):
        out = (C.c_int64 * int(world))() if to_host else None
        _lib.check(self.lib.rbl_zd_return_partition(self._h, int(nmax), int(world), out))
        return [int(x) for x in out] if to_host else None

    def zd_scatter(self, n_back):
        _lib.check(self.lib.rbl_zd_scatter(self._h, int(n_back)))

    # sort-free distributed z-step for banded rank weights (include/rbl.h: rbl_zbd_*)
    def zbd_begin(self):
        """-> (applicable, [clusters that can pool])"""
        a, mask = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.rbl_zbd_begin(self._h, C.byref(a), C.byref(mask)))
        return bool(a.value), [k for k in range(8) if mask.value >> k & 1]

    def zbd_hist(self, p):
        _lib.check(self.lib.rbl_zbd_hist(self._h, int(p)))

    def zbd_scan(self, p):
        _lib.check(self.lib.rbl_zbd_scan(self._h, int(p)))

    def zbd_eval(self, k):
        _lib.check(self.lib.rbl_zbd_eval(self._h, int(k)))

    def zbd_decide(self, k, last, want_settled=True):
        """-> settled (bool; the same on every rank) when want_settled, else None (no host wait)"""
        if not want_settled:
            _lib.check(self.lib.rbl_zbd_decide(self._h, int(k), int(bool(last)), None))
            return None
        st = C.c_int(0)
        _lib.check(self.lib.rbl_zbd_decide(self._h, int(k), int(bool(last)), C.byref(st)))
        return bool(st.value)

    def zbd_root_passes(self):
        return int(self.lib.rbl_zbd_root_passes())

    def zbd_gather(self, k):
        _lib.check(self.lib.rbl_zbd_gather(self._h, int(k)))

    def zbd_finish(self, k, packs_all_ptr, world):
        _lib.check(self.lib.rbl_zbd_finish(self._h, int(k), C.c_void_p(int(packs_all_ptr)), int(world)))

    def zbd_apply(self):
        st = C.c_int(0)
        _lib.check(self.lib.rbl_zbd_apply(self._h, C.byref(st)))
        return st.value

    def zband_status(self):
        """status word of the last sort-free z-step (include/rbl.h: rbl_zband_status); 0 = certified, -1 = none yet"""
        return self.zband_status_split()[0]

    def zband_status_split(self):
        """-> (status word, pooled blocks of that z-step whose value comes from bracket-split sums; -1 = none yet)"""
        st, split = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.rbl_zband_status(self._h, C.byref(st), C.byref(split)))
        return st.value, split.value

    def risk_path(self):
        """which kernels computed the handle's last risk (include/rbl.h: rbl_risk_path): 0 none yet, 1 mean (erm),
        2 sort + dot, 3 banded select"""
        p = C.c_int(0)
        _lib.check(self.lib.rbl_risk_path(self._h, C.byref(p)))
        return p.value

    def pending_reduce(self):
        m = C.c_int(0)
        _lib.check(self.lib.rbl_pending_reduce(self._h, C.byref(m)))
        return m.value

    def risk_from_v(self, v_all_ptr):
        out = C.c_double(0)
        _lib.check(self.lib.rbl_risk_from_v(self._h, C.c_void_p(v_all_ptr), C.byref(out)))
        return out.value

    # -------------------------------------------------------------- measurement
    def profile_kernels(self, enable=True):
        """0/False: no events in the iteration; 1/True: HIP events around the sweep kernels
        (kernel_time()); 2: also around the phases (the ms_* fields of the step statistics)."""
        _lib.check(self.lib.rbl_profile_kernels(self._h, int(enable)))

    def profile_sampling(self, every=1):
        """kernel events on every `every`-th iteration only (include/rbl.h: rbl_profile_sampling)."""
        _lib.check(self.lib.rbl_profile_sampling(self._h, int(every)))

    def reset_kernel_times(self):
        _lib.check(self.lib.rbl_reset_kernel_times(self._h))

    def kernel_samples(self, which):
        """the timed launches of one kernel since the last reset, in launch order (ms)"""
        cnt = C.c_int64(0)
        _lib.check(self.lib.rbl_kernel_samples(self._h, int(which), None, 0, C.byref(cnt)))
        out = np.empty(cnt.value)
        _lib.check(self.lib.rbl_kernel_samples(self._h, int(which), _lib.ptr(out), cnt.value, C.byref(cnt)))
        return out

    def kernel_time(self, which):
        ms, cnt = C.c_double(0), C.c_int64(0)
        _lib.check(self.lib.rbl_kernel_time(self._h, int(which), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


def check_gram_mode(value):
    """``gram`` of ADMMmethod / ADMMgroup / OneVsRest names a route: anything else is an argument error (no device call)"""
    if value not in _lib.GRAM_MODES:
        raise ValueError(f"gram must be one of {list(_lib.GRAM_MODES)}, got {value!r}")


def check_l1_solver(value):
    """``l1_solver`` of ADMMmethod / ADMMgroup / OneVsRest names an l1 w-step: anything else is an argument error"""
    if value not in _lib.L1_SOLVERS:
        raise ValueError(f"l1_solver must be one of {list(_lib.L1_SOLVERS)}, got {value!r}")


def check_share_sparse(value):
    """``share_sparse`` of Group / ADMMgroup / OneVsRest is a bool: anything else is an argument error (no device call)"""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"share_sparse must be True or False, got {value!r}")


class Group:
    """Several Solvers on one data matrix iterated together, the two passes over D shared (include/rbl.h:
    rbl_group_*).  The solvers stay usable on their own after close().  ``share_sparse=True`` opts a group on
    storage "csr" into the shared multi-column sparse passes (RBL_GROUP_SHARE_SPARSE: same iterates bit for bit, the
    entries of D read once per four members); on dense storage it has no effect."""

    def __init__(self, solvers, share_sparse=False):
        self._g = None
        check_share_sparse(share_sparse)
        self.solvers = list(solvers)
        if not self.solvers:
            raise ValueError("Group needs at least one solver")
        if not all(isinstance(s, Solver) and s._h for s in self.solvers):
            raise ValueError("Group members must be live Solver objects")
        self.lib = _lib.load()
        self.k = len(self.solvers)
        arr = (C.c_void_p * self.k)(*[s._h.value for s in self.solvers])
        g = C.c_void_p()
        flags = _lib.GROUP_SHARE_SPARSE if share_sparse else 0
        _lib.check(self.lib.rbl_group_create_opts(arr, self.k, flags, C.byref(g)))
        self._g = g

    def close(self):
        if getattr(self, "_g", None):
            self.lib.rbl_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, want_objective=False):
        """one ADMM iteration of every member that has not converged -> list of RblStats (member order)"""
        st = (_lib.RblStats * self.k)()
        _lib.check(self.lib.rbl_group_step(self._g, 1 if want_objective else 0, st))
        return list(st)

    def solve(self, max_iter=0, want_objective=False):
        """-> (list of final RblStats, list of per-member history dicts)"""
        cap = int(max_iter if max_iter > 0 else max(s.cfg.max_iter for s in self.solvers))
        hist = {k: np.full((self.k, cap), np.nan) for k in ("objective", "primal", "dual", "rho")}
        st = (_lib.RblStats * self.k)()
        iters = np.zeros(self.k, dtype=np.int64)
        _lib.check(self.lib.rbl_group_solve(self._g, cap, 1 if want_objective else 0, st, _lib.ptr(hist["objective"]),
                                            _lib.ptr(hist["primal"]), _lib.ptr(hist["dual"]), _lib.ptr(hist["rho"]),
                                            iters.ctypes.data_as(C.POINTER(C.c_int64)), cap))
        return list(st), [{name: a[i, :int(iters[i])].copy() for name, a in hist.items()} for i in range(self.k)]

    def profile(self, on=True):
        """HIP events around the shared sparse passes of every step (rbl_group_profile); clears the sums"""
        _lib.check(self.lib.rbl_group_profile(self._g, 1 if on else 0))

    def pass_times(self):
        """per-step milliseconds of the shared sparse passes since profile(): dict(v, q, pack, steps)"""
        ms = (C.c_double * 3)()
        steps = C.c_int64(0)
        _lib.check(self.lib.rbl_group_pass_times(self._g, ms, C.byref(steps)))
        n = max(1, steps.value)
        return dict(v=ms[0] / n, q=ms[1] / n, pack=ms[2] / n, steps=steps.value)

    def counters(self):
        kpp = C.c_int(0)
        sv, sq = C.c_int64(0), C.c_int64(0)
        single = np.zeros(self.k, dtype=np.int64)
        _lib.check(self.lib.rbl_group_counters(self._g, C.byref(kpp), C.byref(sv), C.byref(sq),
                                               single.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(k_per_pass=kpp.value, shared_v=sv.value, shared_q=sq.value, single_passes=[int(x) for x in single])


def reg_terms(w, l2_reg, l1_reg):
    """Regulariser of get_arrogate_loss (objective.py:83-86): both terms when both are set."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    r = 0.0
    if l2_reg:
        r += 0.5 * l2_reg * float(np.sum(w ** 2))
    if l1_reg:
        r += 0.5 * l1_reg * float(np.sum(np.abs(w)))
    return r


def isnan(x):
    return isinstance(x, float) and math.isnan(x)
