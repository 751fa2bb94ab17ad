"""Drop-in mirror of the reference's ``src/optim/algorithms.py`` class API
(Optimizer / ADMMmethod / smoothADMMmethod), running the ADMM iteration on MI355X.

Same constructor arguments, methods, attributes, printed fields and error messages as
the reference (citations: reference ``src/optim/algorithms.py``), so ``run_SRM.py`` /
``run_EHRM.py`` / ``run_AoRR_*.py``-style callers work unchanged with this package
directory on ``PYTHONPATH``.  State (w, z, lambda) lives on the GPU; the ``w`` / ``z`` /
``lagrangian`` attributes download it on access.  All arithmetic is done by librbl.so
(include/rbl.h); this file is host glue.  Extra keyword arguments (after the reference's
own): ``storage`` ("f32" default | "f64" strict | "fp16" half the bytes of D, data rounded once to float16 | "csr" a sparse
X stays sparse on the device: float64 entries, sparse passes, of ``standardize`` only "scale"), ``device``;
``l1_weights`` / ``l2_weights`` (a scalar or one value per feature: the regulariser becomes
1/2 sum_j (l1_j |w_j| + l2_j w_j^2) - elastic net, penalty factors, unpenalised coordinates) and ``fit_intercept``
(an unpenalised bias: the library forms the column -y * 1 itself, no host copy of X; the solver has d + 1 coordinates,
``coef_`` / ``intercept_`` split the result while ``w`` and ``final_res()`` keep the full vector); ``standardize`` (the
columns of X are centred and scaled to unit population variance on the device, one rounding into the storage type;
``scale_mean_`` / ``scale_scale_`` hold the vectors, every later matrix of the object - the test set of ``start_store`` -
gets the same scaling, ``unscaled()`` gives the coefficients for raw features; ``standardize="scale"`` divides the columns
by the same standard deviation without centring them - ``scale_mean_`` is all zeros, a sparse X stays sparse, and with
``fit_intercept`` it is the model of full standardisation, the intercept shifted by sum_j w_j mean_j / scale_j; the one
value storage "csr" takes besides False).  X is taken as it is: a NumPy array or
torch CPU tensor of float64 / float32 / float16 is uploaded in its own type without a host copy, a torch tensor on the
solver's GPU is read where it lives (_solver.as_source).  ``sample_weight`` (n values >= 0) and ``class_weight``
("balanced": c_i = n / (2 n_{y_i}), or a dict {+1: a, -1: b}) weigh the rows of an erm problem: F(w) = (1/n) sum_i c_i
loss_i(w) + R(w) (include/rbl.h: rbl_set_row_weights); ``sample_weight_`` holds the resolved vector (None without
weights), ``set_sample_weight(c)`` replaces it between ``main_loop`` calls or iterations.  ``gram`` ("auto" | "dense" |
"none"): the w-step's route.  "dense" forms G = D^T D and solves in Gram space; "none" (storage "csr" only) never forms it
and applies rho D^T D + diag(.) through the sparse passes (CG for l2, FISTA for l1 / elastic net; include/rbl.h:
RBL_CREATE_NO_GRAM) - the route for more than 16 384 columns, where "auto" picks it; everywhere else "auto" is "dense".
A solver on borrowed data (``share_data``) must name the route of the solver that owns them.  ``l1_solver`` ("fista" |
"working_set") of ADMMmethod: the l1 / elastic-net w-step of the "none" route.  "fista" (the default) is FISTA on the
operator; "working_set" solves it exactly on a working set of at most 1024 columns whose sub-Gram matrix is formed from
the entries and kept, and checks the KKT conditions on all columns with one D^T (D w) (include/rbl.h:
RBL_CREATE_WORKING_SET; ``wset_info_`` reports it).  It needs an l1 penalty, storage "csr" and the "none" route.
"""
import time

import numpy as np

try:
    from ... import _lib, _solver
    from .objective import rankbasedObjective
except ImportError:      # package directory on sys.path: imported as ``src.optim.algorithms``
    import _lib
    import _solver
    from src.optim.objective import rankbasedObjective


class _OnDevice:
    """Marker returned by the default sub-problem hooks: the result already sits on the GPU."""
    __slots__ = ()


_ON_DEVICE = _OnDevice()


class Optimizer:
    standardize = False        # False, True or "scale" (set by __init__)

    def __init__(self, X, y, weight_function="erm", loss="binary_cross_entropy", l2_reg=None, l1_reg=None,
                 B=None, n_class=None, args=None, w0=None, max_iter=200, tol=1e-4, storage="f32", device=0,
                 _wstep=None, _smooth_t=1.0, share_data=None, l1_weights=None, l2_weights=None, fit_intercept=False,
                 standardize=False, sample_weight=None, class_weight=None, gram="auto", l1_solver="fista"):
        # argument checks in the reference's order (objective first :22, then :55-68)
        _solver.check_problem(weight_function, loss, B, args)
        _solver.check_gram_mode(gram)
        _solver.check_l1_solver(l1_solver)
        if l1_reg is None and l2_reg is None and l1_weights is None and l2_weights is None:
            raise ValueError("More arguments: l1_reg or l2_reg not l1_reg and l2_reg!")       # :62
        if B is not None and weight_function != "ehrm":
            raise ValueError(f"Unrecognized weight_function '{weight_function}'! Options: ['ehrm']")  # :65-68
        if weight_function == "ehrm" and B is None:
            raise ValueError("ehrm needs the reference point B")
        standardize = _solver.resolve_standardize(standardize)       # False, True or "scale"
        src = _solver.as_source(X, device)              # X in its own type, where it lives: no host copy
        _solver.check_csr_storage(src, storage, standardize)          # storage="csr": a sparse X, no centring
        # per-coordinate penalties / intercept: validated on the host before any device call; None = the scalar path
        pen = _solver.resolve_penalty(src.shape[1], l1_reg, l2_reg, l1_weights, l2_weights, fit_intercept)
        self.fit_intercept = bool(fit_intercept)
        self.standardize = standardize
        self._pen = pen
        # (fit_intercept: the library forms the column of ones, RBL_DATA_ONES_COLUMN)
        self.num_row, self.num_feature = src.shape[0], src.shape[1] + (1 if self.fit_intercept else 0)   # :26-27
        self.reg = pen["reg"] if pen else (l1_reg or l2_reg)                                  # :30
        self.loss = loss                                                                      # :36
        self.tol, self.max_iter = tol, max_iter                                               # :44-45
        self.w_flag = (1 if pen["wstep"] == _lib.WSTEP_L1 else 2) if pen else (1 if l1_reg is not None else 2)  # :57-60
        self.B = B
        self.w_tol = 7e-5                       # :69 (kept for callers; the GPU w-step is exact)
        self.z_maxiter = self.num_row           # :70 (the GPU PAV needs no sweep cap)
        self.store = False                                                                    # :71
        self.weight_function = weight_function                                                # :73
        self.l1_reg, self.l2_reg = l1_reg, l2_reg
        wstep = _wstep if _wstep is not None else (_lib.WSTEP_L1 if self.w_flag == 1 else _lib.WSTEP_L2)
        # the w-step's route: "dense" (Gram space) or "none" (operator w-step, storage "csr"); argument errors come now
        self.gram = _solver.resolve_gram(gram, storage, self.num_feature)
        # the l1 w-step of the gram="none" route: "fista" or "working_set"; its refusals come now, before any device call
        _solver.resolve_l1_solver(l1_solver, wstep == _lib.WSTEP_L1, storage, self.gram)
        self.l1_solver = l1_solver
        # share_data: another solver of this package built on the same X - its device D and DTD are borrowed; a y that
        # differs from that solver's becomes this solver's own labels (include/rbl.h: rbl_set_labels)
        share = None
        y_own = None
        if share_data is not None:
            share = getattr(share_data, "_s", share_data)
            if not isinstance(share, _solver.Solver):
                raise ValueError("share_data must be an ADMMmethod / smoothADMMmethod (or a Solver) on the same (X, y)")
            if (share.n, share.d) != (self.num_row, self.num_feature) or share.n_total != share.n:
                raise ValueError(f"share_data holds a {(share.n_total, share.d)} problem, X is {(self.num_row, self.num_feature)}")
            if share.cfg.storage != _lib.STORAGE.get(storage, -1) or share.cfg.device != int(device):
                raise ValueError("share_data was built with another storage type or device")
            if y is not None:
                y_own = _solver.as_pm1_labels(y, self.num_row)      # shape / +-1 before any device call
        if self.gram == "none" and wstep == _lib.WSTEP_SMOOTH_L1:
            raise ValueError('smoothADMMmethod needs the Gram matrix (its w-step preconditions with diag(G)): it has no '
                             'gram="none" route' + (f", and storage=\"csr\" with {self.num_feature} coordinates has no "
                                                    "other - use ADMMmethod" if gram == "auto" else ""))
        # row weights (erm only): validated on the host before any device call; None = the unweighted path
        self.sample_weight_ = None
        if sample_weight is not None or class_weight is not None:
            if y is None and share is not None:
                y_w = share.labels()                # the labels of the solver whose data are borrowed
            else:
                y_w = y_own if y_own is not None else _solver.as_pm1_labels(y, self.num_row)
            self.sample_weight_ = _solver.resolve_row_weights(y_w, sample_weight, class_weight, weight_function)
        self._s = _solver.Solver(self.num_row, self.num_feature, weight_function, loss, reg=self.reg, wstep=wstep,
                                 B=B, args=args, smooth_t=_smooth_t, tol=tol, max_iter=max_iter, storage=storage,
                                 device=device, share=share, gram=self.gram, l1_solver=l1_solver)
        if share is None:
            if self.standardize == "scale":
                self._s.set_centering(False)         # unit-variance columns, no centring: the mean vector is zeros
            self._s.set_data(src, y, scaling="fit" if self.standardize else "none",
                             ones_column=self.fit_intercept)                                  # :23 D = -y*X
            self._s.gram()                                                                    # :24 DTD
        elif y_own is not None:
            self._s.set_labels(y_own)
        # the scaling of the data this solver runs on (its own, or the one of the solver it borrows from)
        sc = (share if share is not None else self._s).get_scaling() if self.standardize else None
        if self.standardize and sc is None:
            raise ValueError(f"standardize={self.standardize!r}, but share_data was built without it")
        if share is not None:                        # the mode, not just its truth value
            held = False if share.get_scaling() is None else (True if share.get_centering() else "scale")
            if not self.standardize and held:
                raise ValueError(f"standardize=False, but share_data holds standardised data: pass standardize={held!r}")
            if self.standardize != held:
                raise ValueError(f"standardize={self.standardize!r}, but share_data was built with standardize={held!r}")
        self._scaling = sc
        nf = src.shape[1]
        self.scale_mean_ = None if sc is None else sc[0][:nf].copy()
        self.scale_scale_ = None if sc is None else sc[1][:nf].copy()
        if pen:
            self._s.set_penalty(pen["l1"], pen["l2"])
        if self.sample_weight_ is not None:
            self._s.set_row_weights(self.sample_weight_)
        if w0 is not None:                                                                    # :39-40
            w0 = np.asarray(w0, dtype=np.float64).reshape(-1)
            if self.fit_intercept and w0.size == self.num_feature - 1:
                w0 = np.append(w0, 0.0)                 # coefficients only: the intercept starts at 0
            self._s.set_state(w=w0)
        self.objective = rankbasedObjective(None, None, weight_function, loss, l2_reg, l1_reg, B, n_class, args,
                                            _shared_solver=self._s,
                                            _penalty=(pen["l1"], pen["l2"]) if pen else None)  # :22
        self._storage, self._device = storage, device
        self._last = None

    # ---- state views (reference attributes :32-52, :74-75) ---------------------------------
    @property
    def w(self):
        return self._s.get_state(want_z=False, want_lam=False)["w"].reshape(-1, 1)

    @w.setter
    def w(self, value):
        self._s.set_state(w=np.asarray(value, dtype=np.float64).reshape(-1))

    @property
    def coef_(self):
        """the feature coefficients (d,): w without the intercept's coordinate"""
        w = self.w.reshape(-1)
        return w[:-1] if self.fit_intercept else w

    @property
    def intercept_(self):
        """the unpenalised bias (0.0 without fit_intercept)"""
        return float(self.w.reshape(-1)[-1]) if self.fit_intercept else 0.0

    def unscaled(self):
        """(coef, intercept) for raw features: with standardize the model is x_std . w + b, x_std = (x - mean) / scale,
        so coef_j = w_j / scale_j and intercept = b - sum_j w_j mean_j / scale_j (b = 0 without fit_intercept).  Without
        standardize: (coef_, intercept_)."""
        coef, b = self.coef_, self.intercept_
        if self._scaling is None:
            return coef.copy(), b
        coef = coef / self.scale_scale_
        return coef, b - float(np.dot(coef, self.scale_mean_))

    @property
    def z(self):
        return self._s.get_state(want_lam=False)["z"].reshape(-1, 1)

    @z.setter
    def z(self, value):
        if not isinstance(value, _OnDevice):
            self._s.set_state(z=np.asarray(value, dtype=np.float64).reshape(-1))

    @property
    def lagrangian(self):
        return self._s.get_state(want_z=False)["lam"].reshape(-1, 1)

    @lagrangian.setter
    def lagrangian(self, value):
        self._s.set_state(lam=np.asarray(value, dtype=np.float64).reshape(-1))

    @property
    def rho(self):
        return self._s.get_state(want_z=False, want_lam=False)["rho"]

    @rho.setter
    def rho(self, value):
        self._s.set_state(rho=float(value))

    @property
    def sigma_a(self):
        return self.objective.alphas.numpy().reshape(-1)

    @property
    def sigma_b(self):
        return self.objective.betas.numpy().reshape(-1)

    @property
    def gram_info_(self):
        """how G was formed (include/rbl.h: rbl_gram_report) - with share_data, how the sharing solver's was"""
        return self._s.gram_info()

    @property
    def wset_info_(self):
        """the working set after the last w-step (include/rbl.h: rbl_wset_report; l1_solver="working_set" only)"""
        return self._s.wset_info()

    @property
    def D(self):
        return self._s.get_D()

    @property
    def DTD(self):
        if self.gram == "none":
            raise ValueError(f'DTD: this solver runs with gram="none" - it never forms the {self.num_feature} x '
                             f'{self.num_feature} Gram matrix (the w-step applies D^T (D p) through the sparse passes)')
        D = self._s.get_D()
        return D.T @ D

    # ---- logging (:77-86) ------------------------------------------------------------------
    def set_sample_weight(self, c):
        """Replace the row weights (n values >= 0, at least one > 0; None: back to the unweighted problem) - between
        main_loop calls or between iterations; the next z-step uses them.  The logged objective follows."""
        if c is not None:
            c = _solver.resolve_row_weights(np.ones(self.num_row), c, None, self.weight_function)
        self._s.set_row_weights(c)
        self.sample_weight_ = c

    def start_store(self, X, y, weight_function="erm", loss="binary_cross_entropy", B=None, l2_reg=None,
                    l1_reg=None, n_class=None, args=None, _share_data=None, sample_weight_test=None):
        # the test matrix as it is, with the training scaling and the library's own column of ones; the test objective is
        # unweighted unless it gets weights of its own
        self.test_objective = rankbasedObjective(X, y, weight_function, loss, l2_reg, l1_reg, B, n_class, args,
                                                 storage=self._storage, device=self._device, _share_data=_share_data,
                                                 scaling=self._scaling, _center=self.standardize != "scale",
                                                 _ones_column=self.fit_intercept,
                                                 _penalty=(self._pen["l1"], self._pen["l2"]) if self._pen else None,
                                                 sample_weight=sample_weight_test)
        w = self.w
        self._s.profile_kernels(2)     # z_time / w_time below come from HIP events around the phases
        self.w_time = [0]
        self.z_time = [0]
        self.train_losses = [self.objective.get_arrogate_loss(w)]
        self.test_losses = [self.test_objective.get_arrogate_loss(w)]
        self.time_array = [0]
        self.store = True

    # ---- sub-problem hooks (:88-116, :186-207).  A subclass may override ``z_subproblem`` / ``w_subproblem`` (or
    # the ``_z_subproblem`` / ``_w_subproblem`` wrappers the reference's ADMMmethod defines, :186-207) and return
    # its own (n,1) / (d,1) array: main_loop then hands it to the library, which rebuilds what the later
    # phases derive from it (c = z + lambda/rho, ||z||^2; w_prev, the dual residual) - see
    # include/rbl.h: rbl_phase_z_external / rbl_phase_w_external.  The defaults leave the result on the GPU.
    def z_subproblem(self):
        self._s.phase_m()          # m = D w - lambda/rho                          :89
        self._s.phase_z()          # sort + PAV (prox only for erm) + scatter      :92-104
        return _ON_DEVICE

    def w_subproblem(self):
        self._s.phase_q()          # q = D^T (z + lambda/rho)
        self._s.phase_w()          # Gram-space lasso / ridge / smoothed-l1       :109-116, :190-207
        return _ON_DEVICE

    def _z_subproblem(self):
        return self.z_subproblem()

    def _w_subproblem(self):
        return self.w_subproblem()

    # ---- one iteration (:119-164) --------------------------------------------------------------
    def main_loop(self, i, t_start, verbose):
        z = self._z_subproblem()
        if not isinstance(z, _OnDevice):
            self._s.phase_z_external(np.asarray(z, dtype=np.float64).reshape(-1))
        w = self._w_subproblem()
        if not isinstance(w, _OnDevice):
            self._s.phase_w_external(np.asarray(w, dtype=np.float64).reshape(-1))
        need_obj = self.store or verbose
        self._s.phase_dual(want_objective=need_obj)    # v = D w, lambda += rho (z - v)    :132
        st = self._s.phase_finish()                    # residuals, stop test, rho rule    :135-157
        self._last = st
        if self.store:
            self.z_time.append(st.ms_z / 1e3 + self.z_time[i])
            self.w_time.append((st.ms_q + st.ms_w) / 1e3 + self.w_time[i])
        if st.converged:                                                                 # :137-141
            print('algorithm converges within tolerance')
            print('iter_num=', i, 'primal_feasibility: ', st.primal, 'dual_feasibility: ', st.dual)
            print('loss=', st.objective if need_obj else self.objective.get_arrogate_loss(self.w))
            return True
        if verbose and i % 10 == 0:                                                      # :142-145
            print('iter_num=', i, 'primal_feasibility: ', st.primal, 'dual_feasibility: ', st.dual)
            print('loss=', st.objective)
        if self.store:                                                                   # :159-162
            self.train_losses.append(st.objective)
            self.test_losses.append(self.test_objective.get_arrogate_loss(self.w))
            self.time_array.append(time.time() - t_start)
        return False

    def final_res(self):
        if self.store:
            return self.w, self.time_array, self.train_losses, self.test_losses          # :166-168
        raise ValueError("Data was not saved.")                                           # :170


class ADMMmethod(Optimizer):
    def __init__(self, X, y, weight_function="erm", loss="binary_cross_entropy", l2_reg=None, l1_reg=None, B=None,
                 n_class=None, args=None, w0=None, max_iter=200, tol=1e-4, storage="f32", device=0,
                 l1_weights=None, l2_weights=None, fit_intercept=False, standardize=False, sample_weight=None,
                 class_weight=None, gram="auto", l1_solver="fista", share_data=None):
        # (share_data stays the trailing keyword; the eight before it are meant to be given by name)
        super().__init__(X, y, weight_function, loss, l2_reg, l1_reg, B, n_class, args, w0, max_iter, tol,
                         storage=storage, device=device, share_data=share_data, l1_weights=l1_weights,
                         l2_weights=l2_weights, fit_intercept=fit_intercept, standardize=standardize,
                         sample_weight=sample_weight, class_weight=class_weight, gram=gram, l1_solver=l1_solver)

    def start_store(self, X, y, weight_function="erm", loss="binary_cross_entropy", B=None, l2_reg=None,
                    l1_reg=None, n_class=None, args=None, sample_weight_test=None):
        super().start_store(X, y, weight_function, loss, B, l2_reg, l1_reg, n_class, args,
                            sample_weight_test=sample_weight_test)

    def main_loop(self, verbose=True):                                                    # :209-216
        t_start = time.time()
        for i in range(self.max_iter):
            if Optimizer.main_loop(self, i, t_start, verbose):
                break
        return self.w

    def final_res(self):
        return super().final_res()


class smoothADMMmethod(Optimizer):
    def __init__(self, X, y, weight_function="erm", loss="binary_cross_entropy", B=None, l2_reg=None, l1_reg=None,
                 n_class=None, args=None, w0=None, t=1, max_iter=200, tol=1e-4, storage="f32", device=0,
                 l1_weights=None, l2_weights=None, fit_intercept=False, standardize=False, sample_weight=None,
                 class_weight=None, gram="auto", share_data=None):
        if gram not in ("auto", "dense"):
            raise ValueError(f'smoothADMMmethod: gram must be "auto" or "dense", got {gram!r} (the smoothed-l1 w-step '
                             "preconditions with diag(G): it needs the Gram matrix)")
        if l1_weights is not None or l2_weights is not None or fit_intercept:
            raise ValueError("smoothADMMmethod has no per-coordinate penalties: l1_weights, l2_weights and fit_intercept "
                             "belong to ADMMmethod (the smoothed-l1 w-step smooths one scalar l1 norm)")
        wstep = _lib.WSTEP_SMOOTH_L1 if l1_reg is not None else None
        super().__init__(X, y, weight_function, loss, l2_reg, l1_reg, B, n_class, args, w0, max_iter, tol,
                         storage=storage, device=device, _wstep=wstep, _smooth_t=float(t), share_data=share_data,
                         standardize=standardize, sample_weight=sample_weight, class_weight=class_weight, gram=gram)

    @property
    def t(self):
        return self._s.get_state(want_z=False, want_lam=False)["smooth_t"]

    @t.setter
    def t(self, value):
        self._s.set_state(smooth_t=float(value))

    def start_store(self, X, y, weight_function="erm", loss="binary_cross_entropy", B=None, l2_reg=None,
                    l1_reg=None, n_class=None, args=None, sample_weight_test=None):
        super().start_store(X, y, weight_function, loss, B, l2_reg, l1_reg, n_class, args,
                            sample_weight_test=sample_weight_test)

    def main_loop(self, verbose=True):                                                    # :248-260
        t_start = time.time()
        for i in range(self.max_iter):
            # the t schedule of :254-255 is applied inside the library's phase_finish
            if Optimizer.main_loop(self, i, t_start, verbose):
                break
        if self.w_flag == 1:
            self._s.finalize_smooth()                                                      # :257-258
            print('final true loss=', self.objective.get_arrogate_loss(self.w))
        return self.w

    def final_res(self):
        return super().final_res()


class ADMMgroup:
    """Several problems on ONE (X, y) - a regularisation path, superquantile levels, AoRR (k, m) pairs, ADMM beside
    sADMM - iterated together: the data is uploaded once, D and DTD are formed once, and every iteration reads D once
    for several problems in each of its two passes (include/rbl.h: rbl_group_*).

    ``problems``: a list of dicts with the reference's constructor keywords (``weight_function, loss, l2_reg, l1_reg, B,
    args, w0``; ``smooth=True`` and ``t=`` make the member a smoothADMMmethod; ``y=`` gives the member labels of its own
    on the shared X - one-vs-rest, multi-label - default: the group's ``y``).  ``solvers`` are ordinary ADMMmethod /
    smoothADMMmethod objects; start_store / main_loop / final_res mirror the single-solver calls and return lists in
    the order of ``problems``.  ``standardize=True`` (in every problem, like ``fit_intercept``: one data matrix) standardises
    the columns of X on the device.  X is taken as it is (_solver.as_source).  ``share_sparse=True`` (in every problem, like
    ``standardize``: one set of passes; storage "csr"): the members share multi-column sparse passes, four per read of the
    entries, with bit-identical iterates (default off: every member runs its own sparse passes); it has no effect on dense
    storage."""

    _KEYS = ("weight_function", "loss", "l2_reg", "l1_reg", "B", "args", "w0", "smooth", "t", "y", "l1_weights",
             "l2_weights", "fit_intercept", "standardize", "sample_weight", "class_weight", "share_sparse", "gram", "l1_solver")

    def __init__(self, X, y, problems, storage="f32", device=0, max_iter=200, tol=1e-4):
        if not isinstance(problems, (list, tuple)) or len(problems) == 0:
            raise ValueError("ADMMgroup needs a non-empty list of problems")
        if len(problems) > 64:
            raise ValueError("ADMMgroup: at most 64 problems in one group")
        self.problems = []
        for k, pr in enumerate(problems):            # before anything can touch the device (a tensor X)
            if isinstance(pr, dict) and "share_sparse" in pr:
                try:
                    _solver.check_share_sparse(pr["share_sparse"])
                except ValueError as e:
                    raise ValueError(f"problem {k}: {e}") from None
        X = _solver.as_source(X, device)             # once for all members: no copy, or one conversion
        for k, pr in enumerate(problems):            # every argument error before any device call
            if not isinstance(pr, dict):
                raise ValueError(f"problem {k}: expected a dict of constructor keywords")
            unknown = sorted(set(pr) - set(self._KEYS))
            if unknown:
                raise ValueError(f"problem {k}: unknown keyword(s) {unknown}; options: {list(self._KEYS)}")
            pr = dict(pr)
            pr.setdefault("weight_function", "erm")
            pr.setdefault("loss", "binary_cross_entropy")
            try:
                _solver.check_problem(pr["weight_function"], pr["loss"], pr.get("B"), pr.get("args"))
                if all(pr.get(k) is None for k in ("l1_reg", "l2_reg", "l1_weights", "l2_weights")):
                    raise ValueError("More arguments: l1_reg or l2_reg not l1_reg and l2_reg!")
                if pr.get("smooth") and (pr.get("l1_weights") is not None or pr.get("l2_weights") is not None
                                         or pr.get("fit_intercept")):
                    raise ValueError("smooth=True members have no l1_weights, l2_weights or fit_intercept")
                if bool(pr.get("fit_intercept")) != bool(problems[0].get("fit_intercept")):
                    raise ValueError("fit_intercept must be the same for every problem of a group (one data matrix)")
                pr["standardize"] = _solver.resolve_standardize(pr.get("standardize", False))
                if pr["standardize"] != _solver.resolve_standardize(problems[0].get("standardize", False)):
                    raise ValueError("standardize must be the same for every problem of a group (one data matrix)")
                if bool(pr.get("share_sparse")) != bool(problems[0].get("share_sparse")):
                    raise ValueError("share_sparse must be the same for every problem of a group (one set of passes)")
                _solver.check_gram_mode(pr.get("gram", "auto"))
                if pr.get("gram", "auto") != problems[0].get("gram", "auto"):
                    raise ValueError("gram must be the same for every problem of a group (one data matrix, one route)")
                _solver.check_l1_solver(pr.get("l1_solver", "fista"))
                if pr.get("l1_solver", "fista") != problems[0].get("l1_solver", "fista"):
                    raise ValueError("l1_solver must be the same for every problem of a group (a borrower follows its owner)")
                if pr.get("smooth") and pr.get("l1_solver", "fista") != "fista":
                    raise ValueError("smooth=True members have no l1_solver (the smoothed-l1 w-step is not a lasso)")
                if pr.get("smooth") and pr.get("gram", "auto") == "none":
                    raise ValueError('smooth=True members have no gram="none" route (the smoothed-l1 w-step needs diag(G))')
                if storage in _lib.STORAGE:
                    route = _solver.resolve_gram(pr.get("gram", "auto"), storage, X.shape[1] + (1 if pr.get("fit_intercept") else 0))
                pen_k = _solver.resolve_penalty(X.shape[1], pr.get("l1_reg"), pr.get("l2_reg"), pr.get("l1_weights"),
                                                pr.get("l2_weights"), bool(pr.get("fit_intercept")))
                if storage in _lib.STORAGE:
                    has_l1 = pen_k["wstep"] == _lib.WSTEP_L1 if pen_k else pr.get("l1_reg") is not None
                    _solver.resolve_l1_solver(pr.get("l1_solver", "fista"), has_l1, storage, route)
                if pr.get("B") is not None and pr["weight_function"] != "ehrm":
                    raise ValueError(f"Unrecognized weight_function '{pr['weight_function']}'! Options: ['ehrm']")
                if pr["weight_function"] == "ehrm" and pr.get("B") is None:
                    raise ValueError("ehrm needs the reference point B")
                if "t" in pr and not pr.get("smooth"):
                    raise ValueError("t is the smoothing parameter of smooth=True members")
                if pr.get("y") is not None:
                    pr["y"] = _solver.as_pm1_labels(pr["y"], X.shape[0])
                if pr.get("sample_weight") is not None or pr.get("class_weight") is not None:   # row weights: on the host, now
                    _solver.resolve_row_weights(_solver.as_pm1_labels(pr["y"] if pr.get("y") is not None else y, X.shape[0]),
                                                pr.get("sample_weight"), pr.get("class_weight"), pr["weight_function"])
            except ValueError as e:
                raise ValueError(f"problem {k}: {e}") from None
            self.problems.append(pr)
        if storage not in _lib.STORAGE:
            raise ValueError(f"storage must be one of {sorted(_lib.STORAGE)}")
        self.max_iter, self.tol = max_iter, tol
        self.solvers = []
        for pr in self.problems:
            kw = {k: pr.get(k) for k in ("l2_reg", "l1_reg", "B", "args", "w0", "sample_weight", "class_weight")}
            share = self.solvers[0] if self.solvers else None
            yk = pr["y"] if pr.get("y") is not None else y
            if pr.get("smooth"):
                s = smoothADMMmethod(X, yk, pr["weight_function"], pr["loss"], t=pr.get("t", 1), max_iter=max_iter, tol=tol,
                                     storage=storage, device=device, share_data=share, standardize=pr["standardize"],
                                     gram=pr.get("gram", "auto"), **kw)
            else:
                s = ADMMmethod(X, yk, pr["weight_function"], pr["loss"], max_iter=max_iter, tol=tol, storage=storage,
                               device=device, share_data=share, l1_weights=pr.get("l1_weights"),
                               l2_weights=pr.get("l2_weights"), fit_intercept=bool(pr.get("fit_intercept")),
                               standardize=pr["standardize"], gram=pr.get("gram", "auto"),
                               l1_solver=pr.get("l1_solver", "fista"), **kw)
            self.solvers.append(s)
        self._group = _solver.Group([s._s for s in self.solvers], share_sparse=bool(self.problems[0].get("share_sparse")))
        self.store = False
        self.last = [None] * len(self.solvers)
        self.iterations = [0] * len(self.solvers)

    def counters(self):
        return self._group.counters()

    @property
    def gram_info_(self):
        """how the members' one G was formed (include/rbl.h: rbl_gram_report)"""
        return self.solvers[0].gram_info_

    def close(self):
        self._group.close()

    def start_store(self, X_test, y_test):
        """test-set objectives of every member (Optimizer.start_store) on ONE uploaded test matrix.  y_test: one label
        array for all members, or a list of K label arrays when the members carry labels of their own."""
        K = len(self.solvers)
        X_test = _solver.as_source(X_test)           # once for all members (the library checks a tensor's device)
        if isinstance(y_test, (list, tuple)) and len(y_test) > 0 and np.ndim(y_test[0]) >= 1:
            if len(y_test) != K:
                raise ValueError(f"problem {min(len(y_test), K)}: y_test lists {len(y_test)} label arrays for {K} problems")
            n_test = X_test.shape[0]
            ys = []
            for k, yt in enumerate(y_test):
                try:
                    ys.append(_solver.as_pm1_labels(yt, n_test, what="y_test"))
                except ValueError as e:
                    raise ValueError(f"problem {k}: {e}") from None
        else:
            ys = [y_test] * K
        first = None
        for s, pr, yk in zip(self.solvers, self.problems, ys):
            Optimizer.start_store(s, X_test, yk, pr["weight_function"], pr["loss"], pr.get("B"), pr.get("l2_reg"),
                                  pr.get("l1_reg"), None, pr.get("args"), _share_data=first)
            first = first or s.test_objective
        self.store = True

    def main_loop(self, verbose=True):
        """up to max_iter group iterations; a member that converges is frozen where its own main_loop would have
        stopped.  Returns the list of w."""
        t_start = time.time()
        live = [True] * len(self.solvers)
        for i in range(self.max_iter):
            if not any(live):
                break
            stats = self._group.step(want_objective=self.store or verbose)
            for k, (s, st) in enumerate(zip(self.solvers, stats)):
                if not live[k]:
                    continue
                self.last[k] = s._last = st
                self.iterations[k] = i + 1
                if s.store:
                    s.z_time.append(st.ms_z / 1e3 + s.z_time[i])
                    s.w_time.append((st.ms_q + st.ms_w) / 1e3 + s.w_time[i])
                if st.converged:
                    live[k] = False
                    print(f'problem {k}: algorithm converges within tolerance')
                    print('iter_num=', i, 'primal_feasibility: ', st.primal, 'dual_feasibility: ', st.dual)
                    continue
                if verbose and i % 10 == 0:
                    print(f'problem {k}: iter_num=', i, 'primal_feasibility: ', st.primal, 'dual_feasibility: ', st.dual)
                    print('loss=', st.objective)
                if s.store:
                    s.train_losses.append(st.objective)
                    s.test_losses.append(s.test_objective.get_arrogate_loss(s.w))
                    s.time_array.append(time.time() - t_start)
        for s in self.solvers:
            if isinstance(s, smoothADMMmethod) and s.w_flag == 1:
                s._s.finalize_smooth()                                                     # :257-258
        return [s.w for s in self.solvers]

    def final_res(self):
        return [s.final_res() for s in self.solvers]


class OneVsRest:
    """K-class classification as K one-vs-rest rank-based problems on ONE feature matrix: member k has the labels
    y_k = +1 where ``labels == classes_[k]`` and -1 elsewhere; X is uploaded once, D and DTD are formed once and every
    iteration reads D once for several classes in each of its two passes (ADMMgroup with per-member labels,
    include/rbl.h: rbl_set_labels).  The reference's ``n_class`` / multinomial loss has no z-step (its prox is missing),
    so this is the multi-class route of the ADMM.  ``predict`` takes the arg-max of x . w_k over the classes on the
    GPU (rbl_decide_multi).  ``share_sparse=True`` (storage "csr"): the classes share multi-column sparse
    passes (ADMMgroup's ``share_sparse``); default off."""

    standardize = False        # False, True or "scale" (set by __init__)

    def __init__(self, X, labels, weight_function="erm", loss="binary_cross_entropy", l2_reg=None, l1_reg=None, B=None,
                 args=None, storage="f32", device=0, max_iter=200, tol=1e-4, l1_weights=None, l2_weights=None,
                 fit_intercept=False, standardize=False, sample_weight=None, class_weight=None, share_sparse=False,
                 gram="auto", l1_solver="fista"):
        _solver.check_share_sparse(share_sparse)     # before anything touches the device
        _solver.check_gram_mode(gram)
        _solver.check_l1_solver(l1_solver)
        self.standardize = _solver.resolve_standardize(standardize)
        # class_weight="balanced": every member gets the balanced weights of its OWN +-1 labels (one class against the
        # rest is imbalanced by construction); a common sample_weight multiplies into all of them
        Xm = _solver.as_source(X, device)
        self.fit_intercept = bool(fit_intercept)
        lab = np.asarray(labels.detach().cpu().numpy() if hasattr(labels, "detach") else labels).reshape(-1)
        if lab.shape[0] != Xm.shape[0]:
            raise ValueError(f"labels has {lab.shape[0]} entries for {Xm.shape[0]} rows")
        self.classes_ = np.unique(lab)
        if self.classes_.size < 2:
            raise ValueError(f"OneVsRest needs at least 2 classes, labels holds {self.classes_.size}")
        if self.classes_.size > 64:
            raise ValueError(f"OneVsRest: at most 64 classes in one group, labels holds {self.classes_.size}")
        ys = [np.where(lab == c, 1.0, -1.0) for c in self.classes_]
        problems = [dict(weight_function=weight_function, loss=loss, l2_reg=l2_reg, l1_reg=l1_reg, B=B, args=args, y=yk,
                         l1_weights=l1_weights, l2_weights=l2_weights, fit_intercept=self.fit_intercept,
                         standardize=self.standardize, sample_weight=sample_weight, class_weight=class_weight,
                         share_sparse=share_sparse, gram=gram, l1_solver=l1_solver)
                    for yk in ys]
        self._storage, self._device = storage, device
        self.group = ADMMgroup(Xm, ys[0], problems, storage=storage, device=device, max_iter=max_iter, tol=tol)
        first = self.group.solvers[0]
        self._scaling = first._scaling          # the training scaling: predict applies it to its matrix
        self.scale_mean_, self.scale_scale_ = first.scale_mean_, first.scale_scale_
        self.W = None
        self._test = None      # (objective-only solver holding the last test matrix, that matrix)

    def main_loop(self, verbose=True):
        """solves the K problems together -> W of shape (d, K), column k = class classes_[k]"""
        ws = self.group.main_loop(verbose)
        self.W = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1, 1) for w in ws], axis=1)
        return self.W

    @property
    def gram_info_(self):
        """how the classes' one G was formed (include/rbl.h: rbl_gram_report)"""
        return self.group.gram_info_

    def _current_W(self):
        if self.W is None:
            self.W = np.concatenate([s.w.reshape(-1, 1) for s in self.group.solvers], axis=1)
        return self.W

    def predict(self, X_test):
        """class label of every row of X_test: classes_[argmax_k x . w_k] (ties: the first class)"""
        Xt = _solver.as_source(X_test, self._device)
        d = Xt.shape[1] + (1 if self.fit_intercept else 0)     # W holds the intercepts in its last row
        W = self._current_W()
        if d != W.shape[0]:
            raise ValueError(f"X_test has {d} features, the model {W.shape[0]}")
        _solver.check_csr_storage(Xt, self._storage, what="X_test")
        if self._test is None or self._test[1] is not X_test:
            if self._test is not None:
                self._test[0].close()
            t = _solver.Solver(Xt.shape[0], d, "erm", "binary_cross_entropy", storage=self._storage,
                               device=self._device, objective_only=True)
            if self._scaling is not None:
                t.set_scaling(*self._scaling)
                if self.standardize == "scale":
                    t.set_centering(False)
            t.set_data(Xt, np.ones(Xt.shape[0]), scaling="none" if self._scaling is None else "apply",
                       ones_column=self.fit_intercept)
            self._test = (t, X_test)
        return self.classes_[self._test[0].decide_multi(np.ascontiguousarray(W.T))]

    def accuracy(self, X_test, labels_test):
        lab = np.asarray(labels_test.detach().cpu().numpy() if hasattr(labels_test, "detach") else labels_test).reshape(-1)
        pred = self.predict(X_test)
        if lab.shape[0] != pred.shape[0]:
            raise ValueError(f"labels_test has {lab.shape[0]} entries for {pred.shape[0]} rows")
        return float(np.mean(pred == lab))

    def close(self):
        if self._test is not None:
            self._test[0].close()
            self._test = None
        self.group.close()
