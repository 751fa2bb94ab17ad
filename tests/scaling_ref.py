"""NumPy restatement of the column scaling of rbl_set_data_from (include/rbl.h: RBL_SCALE_FIT / RBL_SCALE_APPLY).

fit: per column the mean and the population standard deviation (ddof 0, as sklearn.preprocessing.scale) of the widened
source, two passes in float64; a column of zero variance gets scale 1.  form_D: the matrix the device stores,
D = round_to_storage(-y * ((x - mean) * (1.0 / scale))), one rounding (_lib.storage_round), optionally with the unscaled
column -y * 1 appended (RBL_DATA_ONES_COLUMN)."""
import numpy as np


def fit(X):
    X = np.asarray(X, dtype=np.float64)
    mean = X.sum(axis=0) / X.shape[0]
    var = ((X - mean) ** 2).sum(axis=0) / X.shape[0]
    scale = np.sqrt(var)
    scale[var == 0.0] = 1.0
    return mean, scale


def standardize(X, mean, scale):
    """(x - mean) * (1.0 / scale) in float64: the arithmetic of the forming kernel, before the sign and the rounding"""
    X = np.asarray(X, dtype=np.float64)
    return (X - np.asarray(mean, dtype=np.float64)) * (1.0 / np.asarray(scale, dtype=np.float64))


def form_D(X, y, mean=None, scale=None, storage="f64", ones_column=False):
    import admm_for_rank_based_loss_amd as rbl
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Z = np.asarray(X, dtype=np.float64) if mean is None else standardize(X, mean, scale)
    D = -y[:, None] * Z
    if ones_column:
        D = np.hstack([D, (-y * 1.0)[:, None]])
    return rbl._lib.storage_round(D, storage)
