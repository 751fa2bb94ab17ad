"""Drop-in mirror of the reference's ``src/util/calculate_acc.py``: the
test accuracy the drivers print after a solve (``run_SRM.py:43``), evaluated on the GPU from
one sweep v = D w."""
import numpy as np

try:
    from ... import _solver
except ImportError:      # package directory on sys.path: imported as ``src.util.calculate_acc``
    import _solver


def calculate_accuracy(w, X_test, y_test, threshold=0.5, loss='binary_cross_entropy', scaling=None, storage="f32"):
    """Fraction of rows with prediction == label (reference calculate_acc.py:3-19).
    binary_cross_entropy: predict +1 iff sigmoid(x.w) >= threshold.  hinge: the reference sets
    every prediction to +1 (calculate_acc.py:13-15); mirrored as is.  squared_hinge (not a loss of the reference):
    predict +1 iff x.w >= 0, ``threshold`` is ignored.  X_test is taken as it is (float64 / float32 / float16, host or
    GPU 0).  ``scaling``: (mean, scale) of a solver trained with standardize=True (``scale_mean_``, ``scale_scale_``) -
    X_test is standardised with them on the device; a w with one entry more than X_test has columns carries the
    intercept last.  ``storage``: how the test matrix is held on the device, as in ADMMmethod; "csr" keeps a sparse X_test
    sparse (the dense passes stop at 19 200 columns, the sparse ones at none); with "csr" a ``scaling`` must carry an
    all-zero mean (``standardize="scale"``): the columns are scaled, not centred."""
    if loss not in ('binary_cross_entropy', 'hinge', 'squared_hinge'):
        raise ValueError(f"loss '{loss}' is not supported! Options: ['binary_cross_entropy','hinge','squared_hinge']")
    X = _solver.as_source(X_test, 0)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    ones = scaling is not None and w.size == X.shape[1] + 1
    # storage "csr" takes the vectors of standardize="scale" alone: scaled without centring, so the mean is all zeros
    scale_only = scaling is not None and storage == "csr"
    if scale_only and np.any(np.asarray(scaling[0], dtype=np.float64) != 0.0):
        raise ValueError('scaling with storage="csr": the mean vector must be all zeros (the vectors of a solver trained '
                         'with standardize="scale") - centring the columns makes the test matrix dense')
    s = _solver.Solver(X.shape[0], X.shape[1] + (1 if ones else 0), "erm", loss, objective_only=True, storage=storage)
    try:
        if scaling is not None:
            s.set_scaling(*_solver.as_scaling(scaling[0], scaling[1], s.d, ones))
            if scale_only:
                s.set_centering(False)
        s.set_data(X, y_test, scaling="none" if scaling is None else "apply", ones_column=ones)
        return s.accuracy(w, threshold)
    finally:
        s.close()
