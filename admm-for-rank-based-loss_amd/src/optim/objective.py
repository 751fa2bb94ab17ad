"""Drop-in mirror of the reference's ``src/optim/objective.py`` public surface
(rankbasedObjective, get_weights and the weight generators), evaluated on the GPU.

``rankbasedObjective.get_arrogate_loss(w)`` = sum_i alphas_i * loss_(i)(w) + regulariser
(reference objective.py:71-87): one HBM sweep v = D w, the per-sample loss, a radix sort
when the weights are not constant, and a dot product - all in librbl.so.  ``alphas`` /
``betas`` are torch float64 (n,1) tensors like the reference's (objective.py:49-54).
"""
import numpy as np

try:
    from ... import _lib, _solver
except ImportError:      # package directory on sys.path: imported as ``src.optim.objective``
    import _lib
    import _solver


def get_weights(name, args=None):
    """objective.py:166-187: returns a generator ``n -> torch weights`` (a pair for ehrm)."""
    import torch
    if name not in _lib.WEIGHT:
        if name not in ("erm", "ehrm") and args is None:
            raise ValueError("args for framework is None!")
        raise ValueError(
            f"Unrecognized framework '{name}'! Options: ['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']")
    if name not in ("erm", "ehrm") and args is None:
        raise ValueError("args for framework is None!")
    if name == "ehrm":
        return (lambda n: torch.from_numpy(_lib.k_weights("ehrm", n)[0]),
                lambda n: torch.from_numpy(_lib.k_weights("ehrm", n)[1]))
    return lambda n: torch.from_numpy(_lib.k_weights(name, n, args)[0])


def get_erm_weights(n):
    return get_weights("erm")(n)


def get_extremile_weights(n, r):
    return get_weights("extremile", [r])(n)


def get_superquantile_weights(n, q):
    return get_weights("superquantile", [q])(n)


def get_esrm_weights(n, rho):
    return get_weights("esrm", [rho])(n)


def get_aorr_weights(n, qlow, qup):
    return get_weights("aorr", [qlow, qup])(n)


def get_aorr_dc_weights(n, k, m):
    if k <= m:
        raise ValueError("need args[0] > args[1]!")
    return get_weights("aorr_dc", [k, m])(n)


def get_cpt_weights_a(n):
    return get_weights("ehrm")[0](n)


def get_cpt_weights_b(n):
    return get_weights("ehrm")[1](n)


class rankbasedObjective:
    """objective.py:39-94.  Holds D = -y*X on the device (own handle, or the solver's)."""

    def __init__(self, X, y, weight_function="erm", loss="binary_cross_entropy", l2_reg=None, l1_reg=None,
                 B=None, n_class=None, args=None, storage="f32", device=0, _shared_solver=None, _share_data=None,
                 _penalty=None, scaling=None, _ones_column=False, sample_weight=None, class_weight=None, _center=True):
        # sample_weight / class_weight (erm only): F(w) = (1/n) sum_i c_i loss_i(w) + R(w), _solver.resolve_row_weights
        _solver.check_problem(weight_function, loss, B, args, need_prox=False)
        if loss == "multinomial_cross_entropy":
            raise ValueError("multinomial_cross_entropy is outside the ADMM hot path (binary losses only)")
        self.weight_function_name = weight_function
        self.loss_name = loss
        self.l2_reg, self.l1_reg = l2_reg, l1_reg
        self.B = B
        self.lossB = None if B is None else float(np.logaddexp(0.0, B))     # objective.py:59-63
        self.n_class = n_class
        self.sample_weight_ = None
        if _shared_solver is not None:
            self._s = _shared_solver
            self.n, self.d = self._s.n_total, self._s.d
            if sample_weight is not None or class_weight is not None:
                raise ValueError("a shared solver carries its own row weights: give them to the solver")
        else:
            # X as it is (_solver.as_source).  scaling: (mean, scale) of a solver (its scale_mean_ / scale_scale_, or
            # Solver.get_scaling()) - this matrix is standardised with them on the device; _ones_column: the intercept's
            Xm = _solver.as_source(X, device)
            # _center=False: the vectors of a solver trained with standardize="scale" (an all-zero mean) - scaled, not centred
            scale_only = scaling is not None and not _center
            _solver.check_csr_storage(Xm, storage, "scale" if scale_only else scaling is not None, what="X_test")
            if scale_only and np.any(np.asarray(scaling[0], dtype=np.float64) != 0.0):
                raise ValueError('scaling without centring (standardize="scale") takes an all-zero mean vector')
            self.n, self.d = Xm.shape[0], Xm.shape[1] + (1 if _ones_column else 0)
            # _share_data: another objective on the same (X, y) whose device matrix this one borrows (ADMMgroup)
            share = None if _share_data is None else _share_data._s
            if share is not None and (share.n, share.d) != (self.n, self.d):
                raise ValueError(f"shared data is {(share.n, share.d)}, X is {(self.n, self.d)}")
            y_own = _solver.as_pm1_labels(y, self.n) if share is not None and y is not None else None
            if sample_weight is not None or class_weight is not None:      # on the host, before any device call
                y_w = share.labels() if (y is None and share is not None) else _solver.as_pm1_labels(y, self.n)
                self.sample_weight_ = _solver.resolve_row_weights(y_w, sample_weight, class_weight, weight_function)
            self._s = _solver.Solver(self.n, self.d, weight_function, loss, args=args, B=B, storage=storage,
                                     device=device, objective_only=True, share=share)
            if share is None:
                if scaling is not None:
                    self._s.set_scaling(*_solver.as_scaling(scaling[0], scaling[1], self.d, _ones_column))
                    if scale_only:
                        self._s.set_centering(False)
                self._s.set_data(Xm, y, scaling="none" if scaling is None else "apply", ones_column=_ones_column)
            elif y_own is not None:
                self._s.set_labels(y_own)      # labels of its own on the borrowed matrix (rbl_set_labels)
            if self.sample_weight_ is not None:
                self._s.set_row_weights(self.sample_weight_)
        # per-coordinate penalties (l1, l2) of the solver (ADMMmethod's l1_weights / l2_weights / fit_intercept): the
        # regulariser is then evaluated by the library on this handle (rbl_objective), an own handle is given the vectors
        self._penalty = _penalty
        if _penalty is not None and _shared_solver is None:
            self._s.set_penalty(_penalty[0], _penalty[1])
        self._alphas = self._betas = None

    def _sig(self):
        if self._alphas is None:
            import torch
            a, b = self._s.sigma()
            self._alphas = torch.from_numpy(a).reshape(-1, 1)
            self._betas = self._alphas if self.weight_function_name != "ehrm" else torch.from_numpy(b).reshape(-1, 1)
        return self._alphas, self._betas

    @property
    def alphas(self):
        return self._sig()[0]

    @property
    def betas(self):
        return self._sig()[1]

    def get_arrogate_loss(self, w, include_reg=True):
        """objective.py:71-87 (betas = alphas there, :76, so the EHRM split sums to the same dot)."""
        wv = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
        wv = np.asarray(wv, dtype=np.float64).reshape(-1)
        if include_reg and self._penalty is not None:
            return self._s.objective(wv)
        risk = self._s.risk(wv)
        if include_reg:
            risk += _solver.reg_terms(wv, self.l2_reg, self.l1_reg)
        return risk
