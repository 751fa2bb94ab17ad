"""Drop-in mirror of the reference's ``src/util/fair_metric.py``: the group
fairness statistics ``run_EHRM.py:41`` prints after a solve, evaluated on the GPU (one sweep
v = D w, group-wise confusion counts and the Theil-index sums in one reduction kernel)."""
import numpy as np

try:
    from ... import _solver
except ImportError:      # package directory on sys.path: imported as ``src.util.fair_metric``
    import _solver


def calculate_statistics(w, X_test, label_test, group_test, threshold=0.5, scaling=None):
    """Returns (SPD, DI, EOD, AOD, TI, FNRD) as reference fair_metric.py:3-41 (group 0 = G1,
    group 1 = G2; predictions from sigmoid(x.w) >= threshold).  X_test is taken as it is; ``scaling``: (mean, scale) of a
    solver trained with standardize=True, applied to X_test on the device (calculate_accuracy has the same argument)."""
    X = _solver.as_source(X_test, 0)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    ones = scaling is not None and w.size == X.shape[1] + 1
    s = _solver.Solver(X.shape[0], X.shape[1] + (1 if ones else 0), "erm", "binary_cross_entropy", objective_only=True)
    try:
        if scaling is not None:
            s.set_scaling(*_solver.as_scaling(scaling[0], scaling[1], s.d, ones))
        s.set_data(X, label_test, scaling="none" if scaling is None else "apply", ones_column=ones)
        return s.fair_statistics(w,
                                 np.asarray(group_test, dtype=np.float64).reshape(-1), threshold)
    finally:
        s.close()
