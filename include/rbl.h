/* rbl.h - C ABI of librbl.so: the ADMM inner iteration for rank-based loss
 * minimisation on AMD Instinct MI355X (gfx950), hand-written HIP.
 *
 * This is the drop-in boundary for the hot path of RufengXiao/ADMM-for-rank-based-loss
 * (reference paths below are relative to that repository).  The reference has no
 * FFI layer - its boundary is the Python class API of src/optim/algorithms.py - so
 * every entry point names the reference interface it stands behind; the Python
 * mirror of that class API (admm-for-rank-based-loss_amd/src/optim/algorithms.py)
 * binds these symbols with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions: plain pointers and sizes only; every function returns an int status
 * (0 = ok, <0 = error, message via rbl_last_error()); no exceptions cross the
 * boundary; the library owns all device memory; the caller owns all host buffers;
 * no callbacks.  One solver handle per host thread.  Host arrays are row-major
 * float64 unless stated.  There is NO CPU fallback: every compute entry point
 * fails with RBL_ERR_NO_DEVICE when no gfx950 device is present.
 */
#ifndef RBL_H
#define RBL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBL_VERSION 106

/* status codes */
enum {
    RBL_OK = 0,
    RBL_ERR_INVALID = -1,    /* bad argument / bad configuration (Python side raises ValueError) */
    RBL_ERR_NO_DEVICE = -2,  /* no HIP device: the product path has no CPU fallback */
    RBL_ERR_HIP = -3,        /* a HIP runtime call failed */
    RBL_ERR_STATE = -4,      /* call order violated (e.g. step before set_data) */
    RBL_ERR_NOMEM = -5
};

/* loss: src/optim/objective.py:27-37 (get_loss); the reference's z-step has a prox for the first two
 * (src/util/individual_solver.py:112-123).  RBL_LOSS_SQHINGE, max(0, 1 - y x.w)^2, is this library's own: every prox and
 * every pooled block is closed form.  The ADMM solver, the objective and the rbl_k_* entry points take all
 * three; EHRM (has_B) is BCE only, and the baselines (rbl_bl_create) mirror the reference's competitors: first two only. */
enum { RBL_LOSS_BCE = 0, RBL_LOSS_HINGE = 1, RBL_LOSS_SQHINGE = 2 };

/* weight_function: src/optim/objective.py:166-187 (get_weights) */
enum {
    RBL_W_ERM = 0, RBL_W_EXTREMILE = 1, RBL_W_SUPERQUANTILE = 2, RBL_W_ESRM = 3,
    RBL_W_AORR = 4, RBL_W_AORR_DC = 5, RBL_W_EHRM = 6
};

/* w-step flavour: src/optim/algorithms.py:57-60,190-207 (ADMMmethod) and :238-246
 * (smoothADMMmethod) */
enum { RBL_WSTEP_L1 = 1, RBL_WSTEP_L2 = 2, RBL_WSTEP_SMOOTH_L1 = 3 };

/* element type D = -y*X is stored in (accumulation is always float64).  RBL_STORE_F16 is IEEE binary16: rows are padded
 * to a multiple of 8 elements (f32 / f64: of 4), the upload rounds to nearest even once, and a finite entry that does not
 * fit the format (|x| >= 65520) is rejected by rbl_set_data / rbl_set_data_from (RBL_ERR_INVALID), never clipped. */
enum { RBL_STORE_F32 = 0, RBL_STORE_F64 = 1, RBL_STORE_F16 = 2 };
/* RBL_STORE_CSR: D lives on the device as its non-zero entries only (row form: int64 indptr, int32 columns, fp64 values
 * -y_r * x widened exactly from the source; column form of the same entries for q = D^T c: 24 bytes per entry in all, no
 * n x ld matrix is ever allocated).  The data come through rbl_set_data_csr alone, with RBL_SCALE_NONE (or scaled without centring: rbl_set_centering); at most 2^31 - 1
 * entries (the column of ones included); row-sharded handles (n != n_total) are refused by rbl_create.  ld follows the
 * f64 rule.  The iteration runs the two-pass form (fused = 0) on sparse passes; see DESIGN.md, "Sparse storage". */
enum { RBL_STORE_CSR = 3 };

/* Constructor arguments of Optimizer.__init__ (src/optim/algorithms.py:20-75). */
typedef struct rbl_config {
    int64_t n;              /* rows held by THIS process (its shard of the sample axis) */
    int64_t d;              /* features */
    int64_t n_total;        /* rows of the whole problem (== n on one GPU) */
    int64_t row_offset;     /* global index of this shard's first row */
    int32_t loss;           /* RBL_LOSS_* */
    int32_t weight_function;/* RBL_W_* */
    double  weight_args[2]; /* args list (objective.py:174-183); unused entries 0 */
    int32_t n_weight_args;  /* 0 = args is None */
    int32_t has_B;          /* B is not None (ehrm only, algorithms.py:64-68) */
    double  B;
    int32_t wstep;          /* RBL_WSTEP_* */
    double  reg;            /* l1_reg or l2_reg (algorithms.py:30) */
    double  smooth_t;       /* smoothADMMmethod t (algorithms.py:225,228) */
    double  rho0;           /* <= 0: reference default by weight_function (algorithms.py:47-52) */
    double  tol;            /* stop tolerance (algorithms.py:44,137; reference default 1e-4); taken literally:
                               tol <= 0 never reports convergence (a fixed number of iterations) */
    double  w_tol;          /* inner w-step tolerance; <= 0: library default 1e-13 */
    int32_t max_iter;       /* algorithms.py:45 */
    int32_t storage;        /* RBL_STORE_* */
    int32_t device;         /* HIP device ordinal */
    int32_t objective_only; /* 1: handle used only for rbl_objective (rankbasedObjective) */
} rbl_config;

/* Per-iteration report of Optimizer.main_loop (src/optim/algorithms.py:119-164). */
typedef struct rbl_stats {
    int64_t iter;            /* iterations completed */
    double  primal;          /* ||z - D w||_2           (algorithms.py:135) */
    double  dual;            /* ||w - w_prev||_2        (algorithms.py:136) */
    double  rho;             /* rho used in this iteration */
    double  rho_next;        /* rho after the schedule  (algorithms.py:154-157) */
    double  objective;       /* F(w) after the iteration (objective.py:71-87); NaN if not computed */
    int32_t converged;       /* both residuals < tol    (algorithms.py:137) */
    int32_t inner_iters;     /* w-step inner iterations */
    int32_t ehrm_branch;     /* 0 = a (z<=B), 1 = b (z>=B), -1 = n/a (PAV_cpt.py:222-226) */
    int32_t pav_merges;      /* seam merges performed by the PAV tree, -1 = n/a */
    float   ms_z, ms_q, ms_w, ms_v, ms_total;  /* device time of the phases, HIP events (rbl_profile_kernels level 2) */
    int32_t fused;           /* 1: this iteration's dual update ran in the single-sweep erm kernel */
    int32_t mispredicted;    /* 1: rho was mispredicted, the next z-step is redone unfused */
    int32_t fused_v;         /* 1: rank-weighted iteration whose v = D w, lambda update and primal residual ran in one
                                pass (the v-only mode of the single-sweep kernel) instead of k_gemv + k_dual */
    int32_t host_syncs;      /* times the host waited for the device inside this iteration's library calls
                                (stream waits, blocking copies, the spin on the pinned statistics block) */
    int32_t sort_passes;     /* radix-sort passes the z-step executed (digits shared by all keys are skipped), -1 = n/a */
    int32_t zband;           /* rank-weighted z-step: 0 = sort + merge-tree PAV, 1 = sort-free banded path (piecewise-constant
                                weights), 2 = banded path not certified, redone with the sort; -1 = n/a */
    int32_t wstep_form;      /* how the w-step ran: 0 = batches of launches (CG / nonlinear CG / FISTA), 1 = ONE persistent
                                launch (k_cg_persist / k_ncg_persist), 2 = the exact active-set lasso kernel, 3 = the
                                eigen-decomposition ridge, 4 = the operator route of a handle without a Gram matrix
                                (RBL_CREATE_NO_GRAM: CG / FISTA on rho D^T (D p) + diag(.) p, batches of launches),
                                5 = the working set of RBL_CREATE_WORKING_SET (a w-step that left it reports 4),
                                -1 = an overridden w_subproblem (rbl_phase_w_external) */
} rbl_stats;

typedef struct rbl_solver rbl_solver;

/* ---- lifetime ------------------------------------------------------------------ */
int  rbl_version(void);
/* sizeof(rbl_config) (which = 0) / sizeof(rbl_stats) (which = 1) / sizeof(rbl_wstep_report) (which = 2) / sizeof(rbl_gram_report) (which = 3) as THIS library was compiled: a binding whose
 * structure definitions are older or newer than the library checks them at load time instead of letting rbl_step
 * write past its buffer; -1 for any other `which` */
int  rbl_sizeof(int which);
const char* rbl_last_error(void);
int  rbl_device_count(void);
/* Optimizer.__init__ / rankbasedObjective.__init__ */
int  rbl_create(const rbl_config* cfg, rbl_solver** out);
int  rbl_destroy(rbl_solver* h);
/* rbl_create with options; flags = 0 is rbl_create.
 *   RBL_CREATE_NO_GRAM  (RBL_STORE_CSR only)  The handle never holds G = D^T D.  Every w-step applies
 *     A = rho D^T D + reg I (or + diag(l2), rbl_set_penalty) as an operator, A p = rho D^T (D p) + ..., through the two
 *     sparse passes: warm-started CG for RBL_WSTEP_L2, FISTA with gradient restart for RBL_WSTEP_L1 (per-coordinate
 *     thresholds and free coordinates included; the exact active-set kernel needs G and is used on this route only
 *     through the working set's sub-Gram matrix, RBL_CREATE_WORKING_SET below), with the stop rules
 *     of the Gram route.  rbl_stats.wstep_form is 4.  Nothing of size d^2 is allocated - no G, no eigenbasis, no lasso
 *     workspace - only one more n-vector and d-vectors, so d is not bounded by the Gram route's ld <= 16 384.  The
 *     d-space sums run in a fixed order that depends on ld alone: the iterates do not depend on the grid.
 *     rbl_gram_local forms nothing (rbl_gram_info reports route 0, "no Gram matrix"); rbl_gram_finish takes the step
 *     constant L = 1.02 lambda_max(D^T D) from 100 power-iteration steps through the operator.  The call order is that
 *     of every handle.  The z-step, the dual update, the residuals, the rho schedule, row weights and own labels do not
 *     see G and are what they are elsewhere.  RBL_BUF_G is RBL_ERR_STATE on such a handle.  RBL_ERR_INVALID, with the
 *     reason: a storage type other than RBL_STORE_CSR; RBL_WSTEP_SMOOTH_L1 on a handle that iterates (its preconditioner
 *     is diag(G)); an unknown flag bit.
 * rbl_create_shared on such an owner gives handles of the same kind (their cfg follows the same rules; D_k^T D_k = D^T D
 * for own labels, so the operator is the owner's).
 *   Without the flag, RBL_STORE_CSR with ld > 16 384 on a handle that iterates is RBL_ERR_INVALID at create (the message
 * names RBL_CREATE_NO_GRAM): the Gram route would allocate ld^2 doubles and refuse the first w-step.
 * The presence of this symbol is the capability probe (RBL_VERSION is unchanged). */
#define RBL_CREATE_NO_GRAM 1
/*   RBL_CREATE_WORKING_SET  (with RBL_CREATE_NO_GRAM and cfg.wstep == RBL_WSTEP_L1 only; otherwise RBL_ERR_INVALID with a
 *     message that says which)  The lasso / elastic-net w-step of such a handle (src/optim/algorithms.py:190-202,
 *     src/util/fast_lasso.py) is solved exactly on a working set S of at most 1024 columns: the sub-Gram matrix of S is
 *     formed from the entries once per column and kept (8 MB; dropped when the data change), the restricted problem goes
 *     through the Gram route's active-set kernel (FISTA on the sub-Gram matrix when its active set outgrows the kernel),
 *     and one D^T (D w) - two sparse passes - checks the KKT conditions on ALL columns: column j outside S joins S when
 *     |g_j| - kappa_j > w_tol * max(1, max_j |q_j|), g = D^T D w + (l2/rho) w - q, the largest violation of each chunk of
 *     2048 columns, at most 64 per round, in a fixed order.  rbl_stats.wstep_form is 5; a w-step that S cannot hold
 *     (more than 1024 columns needed, free coordinates l1_j = 0 included) continues with the operator FISTA from where it stands and reports
 *     4.  A warm start whose support does not fit S is replaced by w = 0 - unless the w-step before it left the route
 *     already: then this one goes to the operator FISTA at once.  Without the flag nothing changes: FISTA.
 *     rbl_create_shared on such an owner gives borrowers with a working set of their own under the same rule
 *     (cfg.wstep == RBL_WSTEP_L1, or objective_only).  The presence of rbl_wset_info is the capability probe. */
#define RBL_CREATE_WORKING_SET 2
int  rbl_create_opts(const rbl_config* cfg, uint32_t flags, rbl_solver** out);
/* A second problem on the SAME (X, y): Optimizer.__init__ again with other weight_function / loss / regulariser / args
 * (examples/run_srm.py:57,68 builds ADMMmethod and smoothADMMmethod on one X_train), without algorithms.py:23-24 being
 * paid again.  The handle borrows the owner's device D = -y*X, G = D^T D and what derives from G alone (Lipschitz
 * constant, eigenbasis) and owns only its per-problem state (w, z, lambda, rho, sigma, z-step and w-step workspaces):
 * no upload, no Gram launch.  cfg must agree with the owner on n, d, n_total, row_offset, storage and device
 * (RBL_ERR_INVALID); the owner must have its data and - unless cfg->objective_only - its Gram matrix ready
 * (RBL_ERR_STATE).  The shared buffers are reference-counted: owner and borrowers may be destroyed in any order, the last
 * one frees them.  rbl_set_data, rbl_generate_synthetic, rbl_synth_*, rbl_gram_* on a borrower are RBL_ERR_STATE.  A
 * borrower used alone behaves exactly like a handle built from the same (X, y). */
int  rbl_create_shared(const rbl_config* cfg, rbl_solver* owner, rbl_solver** out);
/* Labels of its own for a borrower: K label vectors on ONE feature matrix (one-vs-rest, multi-label) are K borrowers of
 * one upload.  y: n host doubles, +-1.  Labels are +-1, so with r = y * y_owner the member's D_k = -y_k*X is r*D and its
 * Gram matrix is the owner's; the handle keeps r as one signed char per row (its only extra device memory) and runs the
 * owner's passes in the owner's sign convention (z~ = r z, lambda~ = r lambda, c~ = r c: v = D w, the lambda update, the
 * primal residual and q = D^T c~ are then literally the owner's launches), the sign being taken out where the z-step
 * and the losses look at a row.  Negation is exact: the handle computes bit for bit what a handle built from (X, y)
 * computes on the two-pass paths.  An erm handle with labels of its own runs the two-pass iteration
 * (rbl_stats.fused == 0).  Every host-side entry point speaks the handle's OWN convention (rbl_get_state,
 * rbl_set_state, rbl_phase_z_external, rbl_get_D = -y*X, rbl_get_labels, rbl_objective, rbl_accuracy,
 * rbl_fair_statistics); of the device buffers, RBL_BUF_M holds the true m while RBL_BUF_Z / RBL_BUF_LAM / RBL_BUF_V are
 * in the owner's sign convention.  y equal to the owner's labels leaves an ordinary borrower.  Call it before the
 * first iteration and before the handle joins a group: not a borrower, iter > 0 or member of a live group is
 * RBL_ERR_STATE; a value other than +-1 or a row-sharded handle (n != n_total) is RBL_ERR_INVALID.  Works on
 * objective_only borrowers (a test matrix with per-member test labels). */
int  rbl_set_labels(rbl_solver* h, const double* y);
/* Per-coordinate penalties: the regulariser becomes R(w) = 1/2 sum_j (l1[j] |w_j| + l2[j] w_j^2) in place of
 * reg/2 ||w||_1 or reg/2 ||w||^2 - the elastic net, penalty factors, and coordinates left unpenalised (an intercept:
 * a column of ones with l1 = l2 = 0).  l1 and l2 hold d host doubles each, NULL = all zeros.  The w-step is then
 *     min_w 1/2 w'(G + diag(l2)/rho) w - q'w + sum_j kappa_j |w_j|,   kappa_j = l1[j] / (2 rho):
 * cfg.wstep == RBL_WSTEP_L1 runs the active-set kernel's per-coordinate instance (wstep_form 2; FISTA when the support
 * outgrows it), where a coordinate with l1[j] = 0 is free - it enters when its gradient is non-zero to rounding, is no
 * break point of the line search and is never dropped; cfg.wstep == RBL_WSTEP_L2 (use it when every l1[j] = 0) runs CG
 * on (rho G + diag(l2)) w = rho q (wstep_form 0 or 1; the eigen-decomposition ridge, form 3, needs a multiple of the
 * identity and is not used).  With some l2[j] = 0 that system is only as definite as G: CG keeps its iteration cap.
 * rbl_step, rbl_solve, rbl_phase_w, the w-step rbl_phase_finish enqueues ahead, rbl_group_step, rbl_objective(include_reg)
 * and the logged objective all use the vectors; the z-step, both passes, the residuals and the rho schedule do not see
 * them.  The initial state is untouched: cfg.reg still sets the starting values.  Both NULL, a negative or non-finite
 * entry, or a smoothed-l1 handle (RBL_WSTEP_SMOOTH_L1) is RBL_ERR_INVALID; iter > 0 is RBL_ERR_STATE.  Allowed on owners,
 * borrowers (relabelled ones too), members before they join a group, objective_only handles (so that a logged test
 * objective carries the same R) and row-sharded handles - every rank must pass the same vectors, the w-step is
 * replicated.  The vectors live in the handle's own arena (2 ld doubles). */
int  rbl_set_penalty(rbl_solver* h, const double* l1, const double* l2);
/* the vectors of rbl_set_penalty (d doubles each, either may be NULL); *is_set = 0 and zeros when none were set */
int  rbl_get_penalty(rbl_solver* h, double* l1, double* l2, int* is_set);
/* Row weights of an erm problem: F(w) = (1/n) sum_i c_i loss_i(w) + R(w).  c: n host doubles in the row order of X, each
 * finite and >= 0, at least one > 0; no normalisation is applied.  The weights enter the z-step alone: the element prox
 * of row i runs with sigma_i = c_i * sigma0 (one product; sigma0 = 1.0 / n_total, so c == 1.0 computes the unweighted
 * path's bits) - in the single-sweep pass (rbl_stats.fused stays 1: sigma_i is a third row-wise load, 8 more bytes per
 * row) and in the two-pass z-step.  D, G, the w-step, the dual update, the residuals, the rho schedule and its
 * prediction never see them, so borrowers of one D carry different weights (cross-validation folds as 0/1 weights).  A
 * row with c_i = 0 leaves the problem: z_i = m_i and its multiplier goes to 0.  rbl_objective, rbl_risk_from_v and the
 * logged objective use the weights; rbl_accuracy, rbl_fair_statistics and rbl_decide_multi do not.
 *   c == NULL returns the handle to the unweighted path (its own two n-vectors are freed, nothing shared is).  May be
 * called whenever rbl_set_state may, also between iterations: the next z-step uses the new weights, and what was
 * computed ahead (the z-step of the previous pass, the w-step enqueued ahead of time) is dropped.  rbl_set_labels and a
 * new upload leave the weights as they are (n is fixed per handle).  Works on owners, borrowers (relabelled ones too),
 * group members and objective_only handles.  RBL_ERR_INVALID, with the reason: a weight that is negative or not finite
 * (the message names the first such row), all weights zero, a weight function other than RBL_W_ERM (with weights the
 * sigma of a rank depends on the cumulative weight in sorted order: the PAV z-step does not apply), a row-sharded handle
 * (n != n_total: several devices are out of scope).  The presence of these symbols is the capability probe
 * (RBL_VERSION is unchanged). */
int  rbl_set_row_weights(rbl_solver* h, const double* c /* n, or NULL */);
/* the weights of rbl_set_row_weights (n doubles, may be NULL); *is_set = 0 and ones when none are set */
int  rbl_get_row_weights(rbl_solver* h, double* c, int* is_set);
/* run the library's kernels on this hipStream_t: NULL is the (legacy) default stream,
 * (void*)-1 goes back to the handle's own non-blocking stream (the initial setting) */
int  rbl_set_stream(rbl_solver* h, void* hip_stream);

/* ---- data: D = -y * X (algorithms.py:23), G = D^T D (algorithms.py:24) ---------- */
/* X: n x d host rows of doubles with leading dimension ldx, y: n labels (+-1).  By definition
 *     rbl_set_data(h, X, y, ldx) = rbl_set_data_from(h, X, RBL_DTYPE_F64, RBL_MEM_HOST, ldx, y, RBL_SCALE_NONE, 0)
 * (below): the same checks, messages ("set_data_from: ..."), 64 MB chunks (RBL_UPLOAD_CHUNK_BYTES applies), and
 * rbl_kernel_time(RBL_KERNEL_SRC_FORM) reports its forming pass.  Of a strided source (ldx > d) nothing is read beyond
 * column d of the last row.  RBL_STORE_F16: a finite entry that rounds to +-inf fails the call with RBL_ERR_INVALID (the
 * message counts them and names the first one); the handle is then without data.
 *   A second upload (any of rbl_set_data*, the generator) keeps the iterate - w, z, lambda, rho, iter, smooth_t, penalties,
 * row weights, own labels - and nothing that was computed from the old data: the Gram matrix and what derives from it have
 * to be formed again, D w, the work a single-sweep pass did ahead for the next iteration and a w-step enqueued ahead of
 * time are dropped, on the handle and on every handle that borrows its data (a borrower notices at its next iteration or
 * evaluation).  The next iteration is the one a fresh handle on the new data runs from the same state.  With borrowers
 * the call waits for the whole device before it writes: none of their passes still reads what is replaced. */
int  rbl_set_data(rbl_solver* h, const double* X, const double* y, int64_t ldx);
/* X in the type it has and from where it lives.  X: n rows of d columns (d - 1 with RBL_DATA_ONES_COLUMN: column d - 1 of
 * D is then -y * 1, never scaled, reported as mean 0 / scale 1), row stride ldx ELEMENTS, naturally aligned, element type
 * dtype, in host memory or in memory of the handle's device (checked: anything else is RBL_ERR_INVALID, with a message).
 * y: n host doubles, +-1.  X is read, never modified and never adopted: the caller may free it when the call returns.
 *   RBL_SCALE_NONE   D = round_to_storage(-y * widen(X)): the product is formed in fp64 (widening is exact, y = +-1) and
 *                    rounded once, to nearest even; entries that do not fit RBL_STORE_F16 are rejected (see above).
 *   RBL_SCALE_FIT    per column the mean and the population standard deviation (ddof 0; zero variance: 1) of the widened
 *                    source are formed on the device in fp64, then D = round_to_storage(-y * ((widen(x) - mean) * (1.0 /
 *                    scale))): one rounding into the storage type.  The vectors stay in the handle (rbl_get_scaling) once
 *                    the call has succeeded; a call that fails leaves the handle's earlier vectors, if any, as they were.  The
 *                    sums are shifted by the column's first row and run over fixed blocks of 1024 rows folded in a fixed
 *                    order: the vectors are bit-identical for a host and a device source and for any chunk size.  A
 *                    non-finite statistic is RBL_ERR_INVALID (the column is named).  Row-sharded handles (n != n_total):
 *                    RBL_ERR_INVALID - reduce the column sums in the driver and use RBL_SCALE_APPLY on every rank.
 *   RBL_SCALE_APPLY  the same formula with the vectors of rbl_set_scaling (none set: RBL_ERR_STATE): test matrices,
 *                    shards.
 * A device source is read on the handle's stream (the caller's writes to X must be complete or ordered on the stream given
 * to rbl_set_stream) and the call synchronises before it returns; with RBL_SCALE_FIT it is read twice (statistics, then
 * D).  A host source is pinned in place and streamed over PCIe in chunks of 64 MB (RBL_UPLOAD_CHUNK_BYTES in the
 * environment overrides the size; whole blocks of 1024 rows) in the caller's type - 2, 4 or 8 bytes per entry - and
 * converted on the device; with RBL_SCALE_FIT it crosses PCIe twice.  Borrowers: RBL_ERR_STATE. */
enum { RBL_DTYPE_F64 = 0, RBL_DTYPE_F32 = 1, RBL_DTYPE_F16 = 2 };   /* element type of the caller's X (IEEE binary64/32/16) */
enum { RBL_MEM_HOST = 0, RBL_MEM_DEVICE = 1 };                       /* where X lives; DEVICE = memory of the handle's device */
enum { RBL_SCALE_NONE = 0, RBL_SCALE_FIT = 1, RBL_SCALE_APPLY = 2 };
enum { RBL_DATA_ONES_COLUMN = 1 };                                   /* flags */
int  rbl_set_data_from(rbl_solver* h, const void* X, int dtype, int mem, int64_t ldx /* in elements */,
                       const double* y /* n host doubles, +-1 */, int scaling, int flags);
/* A sparse X in CSR form, expanded on the device: D itself stays dense.  indptr (n + 1 entries) and indices (nnz) are
 * int32 or int64 (index_type, both the same), values (nnz) has element type dtype; all three live in the same memory kind
 * mem and are naturally aligned.  With nnz == 0, indices and values may be NULL.  By definition the call equals
 *     rbl_set_data_from(h, A, dtype, mem, ds, y, scaling, flags)
 * on the dense expansion A of the same element type (ds = d, or d - 1 with RBL_DATA_ONES_COLUMN; implicit entries are
 * +0.0, stored entries keep their bits, -0.0 and explicit zeros included): the same D bit for bit, the same scaling
 * vectors, the same checks and the same messages - the fp16-overflow refusal names row, column and the value found in the
 * source.  dtype, mem, scaling and flags mean what they mean there; borrowers: RBL_ERR_STATE; RBL_SCALE_FIT on a
 * row-sharded handle: RBL_ERR_INVALID.  The arrays are read, never modified and never adopted.
 *   Structure, checked on the host before anything is enqueued (a device indptr is copied to the host once, and that copy
 * plans the chunks): indptr[0] == 0, indptr non-decreasing, indptr[n] == nnz; device arrays must be memory of the handle's
 * device.  Anything else is RBL_ERR_INVALID.
 *   Entries, checked by the expanding kernel before it stores: 0 <= column < ds, and the columns of a row strictly
 * increasing (canonical CSR: duplicates and unsorted rows are refused, never summed).  An offending entry is not written;
 * after the first pass over the source (the statistics pass under RBL_SCALE_FIT, else the forming pass) the call fails
 * with RBL_ERR_INVALID, the message names the smallest offending row, the index and the rule it breaks, and the handle is
 * left without data (a later valid call works).  No index reaches an address before its range test; int64 indices are
 * compared in 64 bits; a row's entry range is clamped to [0, nnz).
 *   Rows are processed in chunks whose DENSE size is 64 MB (RBL_UPLOAD_CHUNK_BYTES overrides it; whole blocks of 1024 rows
 * under RBL_SCALE_FIT) for host and device sources alike: the staging buffer never grows to n x ds.  A host source is
 * pinned in place and only indptr, indices and values cross PCIe (twice under RBL_SCALE_FIT), the next chunk's slices
 * while the current chunk is expanded and consumed.  rbl_kernel_time(RBL_KERNEL_SRC_STATS / RBL_KERNEL_SRC_FORM) report
 * the passes, expansion included.  The presence of this symbol is the capability probe (RBL_VERSION is unchanged). */
/* On a handle with storage RBL_STORE_CSR nothing is expanded: the entries are checked by the same rules (same messages)
 * and stored as they come, value -y_r * x, explicit zeros and -0.0 included; RBL_DATA_ONES_COLUMN appends the entry
 * (d - 1, -y_r) to every row.  Refused with RBL_ERR_INVALID (the handle is left without data): RBL_SCALE_FIT / APPLY
 * with centring on (centring makes D dense; rbl_set_centering(h, 0) below scales without it), nnz (plus n with the column of ones) above 2^31 - 1.  rbl_set_data / rbl_set_data_from and
 * the generator are RBL_ERR_INVALID there.  A second upload regrows the entry buffers under the handles that borrow the
 * data (the device is waited for first; their D pointer stays) and they drop what they computed from the old entries, as
 * after any second upload (rbl_set_data); after an upload that failed they answer RBL_ERR_STATE until a valid one. */
enum { RBL_INDEX_I32 = 0, RBL_INDEX_I64 = 1 };
int  rbl_set_data_csr(rbl_solver* h, const void* indptr /* n + 1 */, const void* indices /* nnz */,
                      const void* values /* nnz, element type dtype */, int64_t nnz, int index_type,
                      int dtype, int mem, const double* y, int scaling, int flags);
/* the column means and scales RBL_SCALE_APPLY uses: d host doubles each (finite, scale > 0); both NULL clears them */
int  rbl_set_scaling(rbl_solver* h, const double* mean, const double* scale);
/* the vectors of RBL_SCALE_FIT / rbl_set_scaling (either may be NULL); *is_set = 0, means 0 and scales 1 when there are none */
int  rbl_get_scaling(rbl_solver* h, double* mean, double* scale, int* is_set);
/* Scale-only standardisation: center = 1 (the default) leaves RBL_SCALE_FIT / APPLY as described above, every bit and
 * message; center = 0 makes them scale the columns WITHOUT centring, from the next upload on:
 *   RBL_SCALE_FIT    scale_j is the same statistic - the population standard deviation about the mean (ddof 0, zero
 *                    variance: 1) - the mean vector is stored as all zeros (rbl_get_scaling reports it so) and
 *                    D = round_to_storage(-y * (widen(x) * (1.0 / scale))), one rounding.  On dense storage the statistics
 *                    pass is the centred one: the scale vector has its bits.
 *   RBL_SCALE_APPLY  the same formula with the scale vector of rbl_set_scaling; a mean vector that is not all zeros is
 *                    RBL_ERR_INVALID at the upload.
 * With fit_intercept this is the model of full standardisation: x_std.w + b = x_scaled.w + (b - sum_j w_j mean_j / s_j).
 *   RBL_STORE_CSR accepts RBL_SCALE_FIT / APPLY when, and only when, centring is off; entries stay entries.  A stored
 * value is fl((-y_r x) * fl(1.0 / scale_col)) in the row form and in the column form alike (both modes scale the stored
 * values after the store: -y_r x is exact, so these are the bits of scaling at store time); explicit zeros and -0.0 keep
 * their bits; the entry (d - 1, -y_r) of RBL_DATA_ONES_COLUMN is never scaled (mean 0, scale 1).  RBL_SCALE_FIT takes the
 * statistics from the column form: per column, with cnt stored entries of n, sh = the first stored x if cnt == n (the
 * shift of the dense statistics: a constant full column has variance exactly 0) else 0, m = sum (x - sh) / n and
 * var = (sum ((x - sh) - m)^2 + (n - cnt) m^2) / n over the stored x = -y_r * value.  Every sum is two-stage - one wave
 * per segment of 2048 entries of the column (lane l adds the entries 2l, 2l + 1, 2l + 128, ... of the segment in order, then
 * a butterfly), then 16 lanes over the column's segments - so the vectors depend on the column's entries alone: not on
 * the grid, the chunk size, the index or value type or where the source lives.  A non-finite statistic is
 * RBL_ERR_INVALID (the column is named).  An objective-only handle builds no column form: RBL_SCALE_FIT is
 * RBL_ERR_INVALID there, RBL_SCALE_APPLY works.  rbl_kernel_time(RBL_KERNEL_SRC_STATS) reports the statistics launches,
 * RBL_KERNEL_SRC_FORM the store pass plus the scaling launches.
 *   Borrowers: rbl_set_centering is RBL_ERR_STATE, as rbl_set_data* is.  The presence of these symbols is the capability
 * probe (RBL_VERSION is unchanged). */
int  rbl_set_centering(rbl_solver* h, int center);
int  rbl_get_centering(rbl_solver* h, int* center);
/* Synthetic two-class data generated on the device (statistics of
 * src/util/load_data.py:101-116), never materialised on the host. */
int  rbl_generate_synthetic(rbl_solver* h, uint64_t seed, double class_sep, double flip_y);
/* sharded form: raw local rows + local column sums (RBL_BUF_COLSTATS, to be summed over
 * ranks), then standardise and scale by -y.  Same matrix for any sharding of the rows.
 * RBL_STORE_F16: the column sums are those of the unrounded draws and the standardised values are regenerated and
 * rounded once - the matrix is the element-wise binary16 rounding of the RBL_STORE_F64 generator's. */
int  rbl_synth_local(rbl_solver* h, uint64_t seed, double class_sep, double flip_y);
int  rbl_synth_finish(rbl_solver* h);
/* labels of the generated rows (+-1), n doubles */
int  rbl_get_labels(rbl_solver* h, double* y_out);
/* Build G and the w-step constants.  For multi-GPU runs call rbl_gram_local(), sum
 * the d*d buffer across ranks (rbl_buffer RBL_BUF_G) and then rbl_gram_finish(). */
int  rbl_gram_local(rbl_solver* h);
int  rbl_gram_finish(rbl_solver* h);
/* how the last rbl_gram_local formed G.  RBL_STORE_CSR has two routes: the dense expansion of row chunks through the fp64
 * MFMA kernel (its cost is the dense n ld^2 whatever the density), and G from the entries (its cost follows
 * pair_products); rbl_csr_gram_route is the rule between them, a function of three integers. */
typedef struct rbl_gram_report {
    int32_t route;          /* 0 none yet, 1 dense storage (f32/f64/f16), 2 csr by dense expansion, 3 csr from the entries */
    int32_t tile_cols;      /* route 3: columns of G per accumulator tile, else 0 */
    int64_t items, batches; /* route 3: work items, batches of columns */
    int64_t pair_products;  /* sum_r k_r (k_r + 1) / 2 (csr), else 0 */
    int64_t dense_products; /* n * ld * (ld + 1) / 2 */
    int64_t transient_bytes;/* what the route allocated and freed */
    float   ms;             /* HIP events around the route's launches alone */
} rbl_gram_report;
int  rbl_gram_info(rbl_solver* h, rbl_gram_report* out);   /* the last rbl_gram_local of h (a borrower: its owner's) */
int  rbl_csr_gram_route(int64_t n, int64_t ld, int64_t pair_products);   /* the rule itself, no device: 2 or 3 */
int  rbl_get_D(rbl_solver* h, double* out /* n x d */);

/* ---- state: w, z, lambda, rho (algorithms.py:32-52); NULL pointers are skipped ----
 * rbl_set_state keeps whatever does not depend on the values it replaces and drops the rest: a new w voids D w, a new
 * lambda the d-space copy of D^T lambda (it is formed again by the next iteration), any of w, z, lambda, rho the work a
 * single-sweep pass did ahead for the next iteration; iter and smooth_t void nothing.  The next iteration is the one a
 * fresh handle on the same data runs from that state. */
int  rbl_get_state(rbl_solver* h, double* w, double* z, double* lam, double* rho, int64_t* iter, double* smooth_t);
int  rbl_set_state(rbl_solver* h, const double* w, const double* z, const double* lam, const double* rho, const int64_t* iter, const double* smooth_t);
int  rbl_get_sigma(rbl_solver* h, double* alphas, double* betas /* n_total each */);

/* ---- the hot path ---------------------------------------------------------------- */
/* One ADMM iteration = Optimizer.main_loop(i, ...) (algorithms.py:119-164).
 * want_objective != 0 also evaluates F(w_{k+1}) from the cached D w (the `store`
 * logging of algorithms.py:159-161). */
int  rbl_step(rbl_solver* h, int want_objective, rbl_stats* out);
/* ADMMmethod.main_loop / smoothADMMmethod.main_loop (algorithms.py:209-216, 248-260):
 * up to max_iter steps, stops on convergence; history arrays (may be NULL) receive
 * one entry per iteration, cap entries each. */
int  rbl_solve(rbl_solver* h, int max_iter, int want_objective, rbl_stats* last,
               double* hist_objective, double* hist_primal, double* hist_dual, double* hist_rho,
               double* hist_time_s, int64_t cap);
/* smoothADMMmethod's final soft-threshold of w by t (algorithms.py:257-258).  It changes w, and is treated like
 * rbl_set_state(w): a handle that iterates on afterwards starts from the thresholded w. */
int  rbl_finalize_smooth(rbl_solver* h);

/* ---- groups: several problems on one data matrix, iterated together ------------------------------------------
 * The reference's experiments are families of problems on one (X, y) - a regularisation path, superquantile levels,
 * AoRR (k, m) pairs, ADMM beside sADMM (examples/run_srm.py:57,68) - each an Optimizer.main_loop of its own
 * (algorithms.py:119-164).  A group runs one such iteration of EVERY member per step and reads D once for
 * k_per_pass members in each of the two n x d passes (Q = D^T [c_1 .. c_K], V = D [w_1 .. w_K]) instead of once per
 * member:  per member rbl_phase_m + rbl_phase_z  ->  shared Q pass  ->  per member rbl_phase_w  ->  shared V pass (with
 * each member's lambda update and primal residual, rho per member)  ->  per member rbl_phase_finish.
 *  - members: an owner and its borrowers (rbl_create_shared), single-process problems (n == n_total), 1 <= k <= 64;
 *    anything else is RBL_ERR_INVALID.  While the group exists its members run on the group's stream; destroy the
 *    group before its members.  After rbl_group_destroy the members are ordinary handles again.
 *  - every member runs the two-pass structure: erm members do not use the single-sweep pass (rbl_stats.fused == 0).
 *    K rank-weighted problems cost 2 ceil(K / k_per_pass) passes against 2 K standalone; K erm problems cost the same
 *    2 ceil(K / k_per_pass) against K standalone single sweeps: with k_per_pass = 4 a group of erm problems is a loss
 *    at K = 1 (2 passes against 1), a tie at K = 2 and pays from K = 3 on (2 against 3, 2 against 4, 4 against 5, ...).
 *  - the shared passes exist for 32 < packets per row <= 512 (128 < ld <= 2048 with fp32 storage, 64 < ld <= 1024 with
 *    fp64, 256 < ld <= 2048 with fp16: the Q pass' column sums bound the width in elements); outside that range a group runs each member's own passes (shared_v == shared_q == 0, counted in
 *    single_passes).  Column k of a shared pass is bit-identical to the member's own single-column pass.
 *  - RBL_STORE_CSR: by default a group on sparse storage runs every member's own two passes (k_per_pass == 1).
 *    rbl_group_create_opts with RBL_GROUP_SHARE_SPARSE opts into shared sparse passes: the entries of D are read once
 *    for up to 4 members - V = D [w_1 .. w_4] with one FMA chain per member and entry, Q = D^T [c_1 .. c_4] on the
 *    members' c interleaved row by row, so that the line gathered for an entry carries every member's value - and every
 *    member's lambda update, residual and logged loss then run as on its own (rbl_phase_dual's unfused kernels).  Every
 *    fp64 sum keeps the order of the single-column sparse pass, so a group with shared sparse passes reproduces the
 *    standalone RBL_STORE_CSR iterates bit for bit, as the dense group does.  k_per_pass is then 4 at every width; the
 *    packed c (4 n doubles) and the segments' partial sums (4 per segment) live in the group and follow a second upload.
 *    On dense storage the flag has no effect: the width rule above alone decides there.
 *  - a member whose z-step was not certified redoes it and its own q with the single-column pass (counted in
 *    single_passes, as is the v = D w a member needs before its first z-step); the others are not disturbed.
 *  - a member that converges (its own tol) is frozen exactly where rbl_solve would have stopped and drops out of the
 *    later passes; rbl_group_solve ends when all have converged or after max_iter steps (<= 0: the members' largest
 *    max_iter).
 *  - host waits per group step: ONE spin on the pinned statistics for all members (booked on the first live member's
 *    rbl_stats.host_syncs) beside what each member's own w-step / uncertified z-step waits for, as in rbl_step.
 * out / last: k entries in member order (a frozen member keeps its last report); hist_*: k x cap, row i = member i,
 * may be NULL; iters: iterations each member ran in this call. */
typedef struct rbl_group rbl_group;
int  rbl_group_create(rbl_solver* const* members, int k, rbl_group** out);
/* rbl_group_create with flags (rbl_group_create is flags == 0); a bit that is not listed here is RBL_ERR_INVALID */
#define RBL_GROUP_SHARE_SPARSE 1   /* RBL_STORE_CSR: shared multi-column sparse passes (above) */
int  rbl_group_create_opts(rbl_solver* const* members, int k, int flags, rbl_group** out);
int  rbl_group_destroy(rbl_group* g);
int  rbl_group_step(rbl_group* g, int want_objective, rbl_stats* out);
int  rbl_group_solve(rbl_group* g, int max_iter, int want_objective, rbl_stats* last,
                     double* hist_objective, double* hist_primal, double* hist_dual, double* hist_rho,
                     int64_t* iters, int64_t cap);
/* k_per_pass: members one shared launch carries (1: no shared passes at this width); shared_v / shared_q: shared
 * launches so far; single_passes[k]: n x d launches each member ran on its own since the group was created */
int  rbl_group_counters(rbl_group* g, int* k_per_pass, int64_t* shared_v, int64_t* shared_q, int64_t* single_passes);
/* Measuring aid (tools/csr_group_bench.py): with on != 0 a group with shared sparse passes puts HIP events around the
 * shared launches of every step; on == 0 stops that; either call clears the sums.  rbl_group_pass_times: ms3 = the
 * summed milliseconds of [the V batches, the Q batches (interleaving included), the first Q batch's interleaving] and
 * the steps they were summed over. */
int  rbl_group_profile(rbl_group* g, int on);
int  rbl_group_pass_times(rbl_group* g, double* ms3, int64_t* steps);
/* The decision of k one-vs-rest classifiers on the rows of `data` (typically an objective_only handle holding a test
 * matrix): cls[i] = argmax_j x_i . w_j, ties to the lowest j.  W: k x d host doubles (row j = w_j), cls: n host int32,
 * 1 <= k <= 64.  The scores come from the groups' multi-column V product (ceil(k / k_per_pass) passes over data's D,
 * the label sign in D = -y*X taken out), each pass followed by a row-wise comparison against the best score so far.
 * A handle with RBL_STORE_CSR takes the multi-column sparse pass, 4 columns per read of the entries: the scores have
 * the bits of the single-column pass, so the classes are the same. */
int  rbl_decide_multi(rbl_solver* data, int k, const double* W, int32_t* cls);
/* rankbasedObjective.get_arrogate_loss(w) (objective.py:71-87); w: d host doubles */
int  rbl_objective(rbl_solver* h, const double* w, int include_reg, double* out);

/* calculate_accuracy(w, X, y, threshold, loss) of src/util/calculate_acc.py:3-19 on this handle's
 * rows.  BCE: predict +1 iff sigmoid(x.w) >= threshold.  Hinge mirrors the reference's quirk: every prediction is +1.
 * Squared hinge (not in the reference, nothing to mirror): predict +1 iff x.w >= 0; threshold is ignored. */
int  rbl_accuracy(rbl_solver* h, const double* w, double threshold, double* out);
/* calculate_statistics(w, X, label, group, threshold) of src/util/fair_metric.py:3-41 on this
 * handle's rows: out6 = {SPD, DI, EOD, AOD, TI, FNRD}; group: n doubles (0 / 1) */
int  rbl_fair_statistics(rbl_solver* h, const double* w, const double* group, double threshold, double* out6);

/* ---- phase API (one process per GPU; the host does the collectives in between) ---- */
/* A: m = D w - lambda/rho for the local rows (algorithms.py:89) -> RBL_BUF_M */
int  rbl_phase_m(rbl_solver* h);
/* B: z-step (algorithms.py:92-104).  m_all_dev: device pointer to the n_total gathered
 * m values (rank order) or NULL when n == n_total or weight_function == erm. */
int  rbl_phase_z(rbl_solver* h, const void* m_all_dev);
/* B': the caller's own z-step (an overridden Optimizer.z_subproblem that returns an array, algorithms.py:88-106 /
 * :186-188): z (n host doubles, this process's rows) replaces the library's; everything the later phases derive
 * from z is rebuilt.  Runs rbl_phase_m first if the iteration has not been opened yet. */
int  rbl_phase_z_external(rbl_solver* h, const double* z);
/* D': the caller's own w-step (an overridden w_subproblem, algorithms.py:109-116): w (d host doubles, identical
 * on every rank) becomes w_{k+1}; the previous iterate is kept for the dual residual.  Call after rbl_phase_q. */
int  rbl_phase_w_external(rbl_solver* h, const double* w);
/* C: local q = D^T (z + lambda/rho) -> RBL_BUF_Q (d doubles, to be summed over ranks) */
int  rbl_phase_q(rbl_solver* h);
/* D: replicated w-step from the summed q (algorithms.py:109-116,190-207) */
int  rbl_phase_w(rbl_solver* h);
/* E: v = D w, lambda += rho (z - v), local partial sums -> RBL_BUF_RED (to be summed) */
int  rbl_phase_dual(rbl_solver* h, int want_objective);
/* F: residual norms, stop test, rho schedule (algorithms.py:135-157) */
int  rbl_phase_finish(rbl_solver* h, rbl_stats* out);

/* device buffers the host may pass to a collective */
enum { RBL_BUF_M = 0, RBL_BUF_Q = 1, RBL_BUF_RED = 2, RBL_BUF_G = 3, RBL_BUF_V = 4, RBL_BUF_Z = 5,
       RBL_BUF_LAM = 6, RBL_BUF_W = 7, RBL_BUF_COLSTATS = 8,
       /* distributed z-step; the count returned is in ELEMENTS of the type given here */
       RBL_BUF_ZD_SKEYS = 16,  /* int64 x n       sorted keys of the local rows (send)            */
       RBL_BUF_ZD_SIDS = 17,   /* int32 x n       their global row ids (send)                      */
       RBL_BUF_ZD_RKEYS = 18,  /* int64 x n_total keys received for the own range (capacity)       */
       RBL_BUF_ZD_RIDS = 19,   /* int32 x n_total row ids received                                 */
       RBL_BUF_ZD_SMALL = 20,  /* double x 16384  samples [0,256) | bounds [256,259) | EHRM sums
                                  [260,262) | candidates [320,384) | partial sums [512,12800) |
                                  seam sums [12800, ...)                                           */
       RBL_BUF_ZD_BIDS = 21,   /* int32 x n_total row ids of the chunk, grouped by owner (send back) */
       RBL_BUF_ZD_BU = 22,     /* double x n_total their block values (send back)                  */
       RBL_BUF_ZD_ZIDS = 23,   /* int32 x n       row ids received back                            */
       RBL_BUF_ZD_ZU = 24,     /* double x n      block values received back                       */
       RBL_BUF_ZD_COUNTS = 25, /* int64 x 64      rows of the local sorted run that go to each rank (rbl_zd_partition) */
       /* sort-free z-step for banded rank weights, sharded rows (rbl_zbd_*) */
       RBL_BUF_ZB_HIST = 26,   /* int32 x 12288   digit histograms of one select pass (to be SUMMED over the ranks)   */
       RBL_BUF_ZB_TOT = 27,    /* double x 64     block sums of one root pass (to be SUMMED over the ranks)           */
       RBL_BUF_ZB_PACK = 28    /* double x 2049   [count | undecided elements] of this rank (to be ALL-GATHERED)       */ };
int  rbl_buffer(rbl_solver* h, int which, void** dev_ptr, int64_t* n_doubles);
/* ---- distributed z-step for rank-weighted problems on several GPUs ---------------------------
 * (no reference counterpart: the reference is single-process; what is distributed is
 * algorithms.py:88-106.  Driver: admm-for-rank-based-loss_amd/dist.py:_z_distributed; CPU
 * restatement of every call: oracle/zdist.py.)  After rbl_phase_m:
 *   rbl_zd_sort_local        sort the local m (payload: global row id); ZD_SMALL[0,nsamples) = regular samples (NaN = none)
 *   rbl_zd_partition         splitters (nparts-1 doubles, device) -> how many sorted rows go to each rank: left in
 *                            RBL_BUF_ZD_COUNTS on the device (all-gathered there: ONE host wait for the whole count
 *                            matrix); send_counts != NULL additionally downloads them (a host wait of its own)
 *   [all-to-all of ZD_SKEYS / ZD_SIDS into ZD_RKEYS / ZD_RIDS]
 *   rbl_zd_prepare           sort the received chunk (n_recv rows, first sorted position sigma_off), prefix sums;
 *                            ZD_SMALL[260,262) = this chunk's EHRM branch sums (to be summed over ranks)
 *   rbl_zd_pav               exact PAV of the chunk (EHRM: branch from the summed values)
 *   per level of the merge tree over ranks:
 *     rbl_zd_bounds          ZD_SMALL[256,259) = (u_first, u_last, count)          [all-gather]
 *     rbl_zd_seam_setup      this rank's seam / side / violation from all bounds
 *     rounds x { rbl_zd_seam_propose -> ZD_SMALL[320,320+K)                         [all-gather]
 *                rbl_zd_seam_eval    -> ZD_SMALL[512,512+3*world*K)                 [all-reduce] }
 *     rbl_zd_seam_sums       ZD_SMALL[12800,12800+3*nseams)                        [all-reduce]
 *     rbl_zd_seam_fill       pooled block value onto this rank's pooled positions
 *   rbl_zd_return_partition  (row id, value) grouped by owner into ZD_BIDS / ZD_BU.  counts == NULL: no host wait - the
 *                            count matrix of the return trip is the transpose of the forward one, which the driver
 *                            holds; counts != NULL downloads them (and the seam-search error flag, otherwise
 *                            reported by rbl_phase_finish)
 *   [all-to-all into ZD_ZIDS / ZD_ZU]
 *   rbl_zd_scatter           z of the local rows; then rbl_phase_q as usual.
 * Logged objective of rank weights (sum_i sigma_i loss_(i), objective.py:73-82) by the same sample sort:
 *   rbl_zd_sort_losses       sort the local per-sample losses (keys only) + samples; rbl_zd_partition;
 *   [all-to-all of ZD_SKEYS into ZD_RKEYS]; rbl_zd_risk -> ZD_SMALL[264] = this chunk's share [all-reduce]. */
int  rbl_zd_sort_local(rbl_solver* h, int nsamples);
int  rbl_zd_partition(rbl_solver* h, const void* splitters_dev, int nparts, int64_t* send_counts);
int  rbl_zd_sort_losses(rbl_solver* h, int nsamples);
int  rbl_zd_risk(rbl_solver* h, int64_t n_recv, int64_t sigma_off);
int  rbl_zd_prepare(rbl_solver* h, int64_t n_recv, int64_t sigma_off);
int  rbl_zd_pav(rbl_solver* h, const void* fvals_total_dev);
int  rbl_zd_bounds(rbl_solver* h);
int  rbl_zd_seam_setup(rbl_solver* h, int rank, int world, int level, const void* bounds_all_dev);
int  rbl_zd_seam_propose(rbl_solver* h, int K, const void* cand_all_prev_dev, const void* part_sum_prev_dev);
int  rbl_zd_seam_eval(rbl_solver* h, int K, const void* cand_all_dev);
int  rbl_zd_seam_sums(rbl_solver* h, int K, const void* cand_all_prev_dev, const void* part_sum_prev_dev, int nseams);
int  rbl_zd_seam_fill(rbl_solver* h, const void* sums_total_dev);
int  rbl_zd_return_partition(rbl_solver* h, int64_t nmax, int world, int64_t* counts);
int  rbl_zd_scatter(rbl_solver* h, int64_t n_back);

/* Distributed z-step WITHOUT a sort for rank weights that are constant on a few bands (superquantile, aorr, aorr_dc;
 * src/optim/objective.py:108-145) - the reference's z_subproblem (algorithms.py:96-104) for row-sharded m.  No sample
 * sort, no all-to-all, no merge tree: the keys at the band edges by a radix select on histograms summed over the ranks,
 * the pooled block's value as the root of the pooled derivative from sums summed over the ranks, the last undecided
 * elements gathered and settled identically on every rank.  After rbl_phase_m:
 *   rbl_zbd_begin     *applicable = 0: not such weights / iteration 0 / pausing after an uncertified step -> rbl_zd_*.
 *                     *root_clusters: bit k set = band edge k can pool.
 *   for pass 0..5:    rbl_zbd_hist(pass); SUM RBL_BUF_ZB_HIST over the ranks; rbl_zbd_scan(pass)
 *   for every set bit k, up to rbl_zbd_root_passes() times:  rbl_zbd_eval(k); SUM RBL_BUF_ZB_TOT;
 *                     rbl_zbd_decide(k, last = final time, &settled) - settled != 0 (the same on every rank: the state is
 *                     a function of the summed totals; one host wait on a pinned word): no further pass for this k.
 *                     In steady state the first pass settles (its candidates sit around a prediction from the last
 *                     block values).  settled = NULL: no host wait, the caller issues all passes (spare ones are idle).
 *                     then rbl_zbd_gather(k); ALL-GATHER RBL_BUF_ZB_PACK; rbl_zbd_finish(k, gathered, world)
 *   rbl_zbd_apply     z and c = z + lambda/rho of the local rows; *status = 0: certified (go on with rbl_phase_q),
 *                     otherwise every rank got the same non-zero status: run rbl_zd_* for this iteration.            */
int  rbl_zbd_begin(rbl_solver* h, int* applicable, int* root_clusters);
int  rbl_zbd_hist(rbl_solver* h, int pass);
int  rbl_zbd_scan(rbl_solver* h, int pass);
int  rbl_zbd_eval(rbl_solver* h, int k);
int  rbl_zbd_decide(rbl_solver* h, int k, int last, int* settled);
int  rbl_zbd_root_passes(void);
int  rbl_zbd_gather(rbl_solver* h, int k);
int  rbl_zbd_finish(rbl_solver* h, int k, const void* packs_all_dev, int world);
int  rbl_zbd_apply(rbl_solver* h, int* status);
/* read-only (tests, diagnostics): the status word of this handle's last sort-free z-step, single handle or sharded -
 * 0 certified, 1 keys tied across a band edge, 2 select failed, 3 too many key prefixes, 4 bracket lost, 5 unresolved
 * after the root passes, 6 / 7 a block swallows the inner band below / above, 8 a block on one side of a single-rank
 * band, 9 two blocks meet; -1: the handle has not run one.  A verdict still pending is settled first, as by any other
 * entry that looks at the state (rbl_stats.zband tells the path, this tells why a step was redone).  split (may be
 * NULL): how many pooled blocks of that step took their value from sums that were split by the root bracket (the last
 * bit of such a value depends on the hint of the steps before) and not from the pass over the certified block alone;
 * 0 on a certified single-handle step unless an element sits within rounding of the block's edge, every block on the
 * sharded path, which has no such pass.  It changes nothing in the iterate, but like every entry it is a call between
 * phases: a w-step computed ahead of time is discarded (w_prev is copied back, the stream is synchronised). */
int  rbl_zband_status(rbl_solver* h, int* status, int* split);
/* read-only (tests, diagnostics): which kernels computed this handle's last risk sum_i sigma_i loss_(i) (rbl_objective,
 * rbl_risk_from_v, the objective of a step) - 0 none yet, 1 the mean (erm), 2 sort + dot with sigma, 3 the banded select
 * (no sort; only after the handle's first rank-weighted z-step has classified sigma).  Nothing is dispatched on it. */
int  rbl_risk_path(rbl_solver* h, int* path);

/* RBL_BUF_Q is the whole exchange buffer [q (ld) | D^T lambda seed (ld) | ||z||^2 | primal^2 |
 * sum loss]; RBL_BUF_RED is its 2-double tail.  After rbl_phase_q and after rbl_phase_dual this
 * tells which part awaits the sum over ranks: bit 0 = the first 2 ld + 1 doubles, bit 1 = the
 * tail; mask 3 = one collective over the whole buffer (single-sweep erm iterations). */
int  rbl_pending_reduce(rbl_solver* h, int* mask);
/* sum_i sigma_i * loss_(i) of n_total gathered values of v = D w on the device
 * (objective.py:73-81 without the regulariser) */
int  rbl_risk_from_v(rbl_solver* h, const void* v_all_dev, double* out);
/* padded leading dimension of D / G / q / w buffers, CU count, Lipschitz constant of G */
int  rbl_info(rbl_solver* h, int64_t* ld, int* num_cu, double* lipschitz);

/* ---- measurement ------------------------------------------------------------------ */
/* accumulated HIP-event time of the two n x d sweep kernels since the last reset */
enum { RBL_KERNEL_GEMV = 0, RBL_KERNEL_GEMVT = 1, RBL_KERNEL_SWEEP_ERM = 2 };
/* the two passes of the last rbl_set_data_from (or rbl_set_data: the forming pass) on the handle's stream (not
 * accumulated; launches = 1 if the pass ran):
 * the column statistics of RBL_SCALE_FIT and the forming of D.  Device source: the kernels alone; host source: the
 * pipelined pass, the copies it waits for included. */
enum { RBL_KERNEL_SRC_STATS = 3, RBL_KERNEL_SRC_FORM = 4 };
int  rbl_kernel_time(rbl_solver* h, int which, double* total_ms, int64_t* launches);
int  rbl_reset_kernel_times(rbl_solver* h);
/* The timed launches of one kernel since the last reset, one by one in launch order (milliseconds): the first
 * min(cap, *count) of them are written to out_ms, *count is how many there are.  bench.py reports the first and
 * the last of the timed region and the median of its last third beside the mean (the reference keeps a
 * cumulative time stamp per iteration, algorithms.py:162; this is its per-launch counterpart). */
int  rbl_kernel_samples(rbl_solver* h, int which, double* out_ms, int64_t cap, int64_t* count);
/* enable: 0 = no HIP events inside the iteration (default: an event record costs ~5 us of stream
 * time), 1 = events around the sweep kernels (rbl_kernel_time), 2 = also around the phases (the
 * ms_* fields of rbl_stats, 0 otherwise) */
int  rbl_profile_kernels(rbl_solver* h, int enable);
/* kernel events (level >= 1) on every `every`-th iteration only; default 1.  With several GPUs the pass
 * of a rank is short (0.55 ms at 8 x 750 000 rows) and two events per iteration are 2 % of it. */
int  rbl_profile_sampling(rbl_solver* h, int every);

/* ---- kernel-level entry points over host buffers (parity tests call these) -------- */
/* element prox (src/util/individual_solver.py:112-123; RBL_LOSS_SQHINGE: the closed form); loss: any RBL_LOSS_* */
int  rbl_k_prox(int loss, int64_t n, const double* sigma, double rho, const double* m, double* out);
/* stable ascending sort of float64 keys with index payload (algorithms.py:92-93) */
int  rbl_k_sort(int64_t n, const double* keys, double* sorted_keys, uint32_t* perm);
/* the z-step's sort with 32-bit keys, exactly its launches: range of m -> fixed-point keys on [min m, max m] -> four
 * radix passes -> fix-up of the runs of equal keys into (m, row id) order.  ids[p] = idx_off + row at sorted position
 * p, m_sorted[p] = its m (the input's bits); *flag = 1: a run of more than 32 equal keys - m_sorted and ids are then
 * meaningless (a solve redoes that z-step with rbl_k_sort's 64-bit keys).  n + idx_off <= 2^32.
 * Signed zeros: the fix-up compares m numerically, so -0.0 and +0.0 tie and keep their row order (as NumPy's stable
 * argsort does); rbl_k_sort orders the bit patterns and puts every -0.0 before every +0.0.  The z-step's result does
 * not depend on it: both zeros are the same m.  NaN in m is not supported (a solve has diverged by then). */
int  rbl_k_sort32(int64_t n, const double* m, uint32_t idx_off, double* m_sorted, uint32_t* ids, int* flag);
/* generalised PAV on sorted m (src/util/pav.py:93-178); loss: any RBL_LOSS_* */
int  rbl_k_pav(int loss, int64_t n, const double* sigma, double rho, const double* m_sorted,
               double* out, int64_t* n_merges);
/* EHRM z-step on sorted m (src/util/PAV_cpt.py:169-293): branch -1 = choose by the
 * singleton-stage scalar test, 0 = a, 1 = b; *branch_out receives the choice */
int  rbl_k_pav_ehrm(int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho,
                    const double* m_sorted, int branch, double* out, int* branch_out);
/* ncalls successive PAV solves on ONE workspace, which carries the upper seams' hints, the
 * barrier parity and the EHRM speculated branch from one call to the next as a solver handle
 * does between z-steps.  m_sorted and out: ncalls x n.  sigma_b != NULL: EHRM (BCE only; the
 * branch is chosen per call, the EHRM clip is applied to out, branch_out[call] receives it).
 * upper selects how the levels above the 2048-position tile run (RBL_PAV_UPPER_*, whatever
 * RBL_PAV_UPPER_PERSIST says).  counters (ncalls x 4, optional): merges, bit mask of the upper
 * levels the persistent kernel looked at, its long (cooperative) fills and its status; the last
 * three are 0 on the two-launch path. */
enum { RBL_PAV_UPPER_PERSIST = 1, RBL_PAV_UPPER_TWO_LAUNCH = 2 };
int  rbl_k_pav_seq(int loss, int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho,
                   int ncalls, const double* m_sorted, int upper, double* out, int* branch_out,
                   uint32_t* counters);
/* v = D w and q = D^T c on a host matrix (storage: RBL_STORE_*) */
int  rbl_k_gemv(int storage, int64_t n, int64_t d, const double* D, const double* w, double* v);
int  rbl_k_gemvt(int storage, int64_t n, int64_t d, const double* D, const double* c, double* q);
/* V = D [w_1 .. w_k] and Q = D^T [c_1 .. c_k] with the multi-column passes of a group (W: k x d, V: k x n, C: k x n,
 * Q: k x d, row j = column j; 1 <= k <= 64; widths outside the shared kernels' range run the single-column pass per
 * column) - algorithms.py:89,132 / :192 for k problems at once */
int  rbl_k_gemv_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* W, double* V);
int  rbl_k_gemvt_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* C, double* Q);
/* The row-streaming passes on prescribed inputs, with a caller-chosen grid: the launchers a solve runs, unchanged, with
 * `num_cu` in the place of the device's CU count (1 <= num_cu <= that count, else RBL_ERR_INVALID).  A wave (a
 * workgroup of the wide kernel) takes the super-batches gw, gw + GW, ... of S*R rows, so with num_cu = 1 it loops after
 * a few hundred (about fifty) rows.  Host fp64 in and out; D is rounded to `storage` (RBL_STORE_F32 / F64 / F16).
 * instance (5 ints, optional) receives which kernel instance ran: kind (0 wave-per-row, 1 workgroup-per-row), P (packets
 * per lane) or PT (packets per thread), R rows per sub-batch, S sub-batches per super-batch, blocks launched.
 * Every row-wise output is preset to NaN on the device and has a guard behind row n: a row the pass does not write comes
 * back as NaN, a write past n is RBL_ERR_STATE.
 *   rbl_k_sweep_erm      the single-sweep pass (sweep_erm.hip lines 5-9): lam_out = lam + rho (z_old - D w), z_new =
 *                        prox(sigma0, rho_next, v - lam_out / rho_next), q = D^T (z_new + lam_out / rho_next), *primal2
 *                        = sum (z_old - v)^2, *zz = sum z_new^2.  rho_next is what the solver predicts on the device
 *                        (pred[0]).  want_v = 0: the pass without the store of v (no objective logging); v may be NULL.
 *                        Widths outside the single-sweep kernels' range are RBL_ERR_INVALID.
 *   rbl_k_sweep_v        v = D w, lam_out = lam + rho (z - v), *primal2 = sum (z - v)^2 (the V-only mode)
 *   rbl_k_sweep_q        q = D^T c through the Q-only mode - its widths only (rbl_k_gemvt takes every width and says
 *                        nothing about the kernel that ran)
 *   rbl_k_sweep_v_multi  k = 1..4 columns in one launch (W: k x d, Z, LAM: k x n, rho[k]); primal2[k].  LAM_out and V
 *                        are 4 x n: rows >= k are buffers of this entry that no launch is told about (the launcher gives
 *                        the kernel's unused slots column 0's pointers), so their NaN says only that no column was
 *                        written past its n rows - not that the kernel skipped the stores of the slots >= k
 *   rbl_k_sweep_q_multi  Q = D^T [c_1 .. c_k], C: k x n, Q: k x d, k = 1..4 */
int  rbl_k_sweep_erm(int storage, int loss, int64_t n, int64_t d, const double* D, const double* w, const double* z_old,
                     const double* lam, double sigma0, double rho, double rho_next, int num_cu, int want_v,
                     double* lam_out, double* v, double* z_new, double* q, double* primal2, double* zz, int* instance);
/* rbl_k_sweep_erm with one sigma per row (sigma: n host doubles, sigma_i = c_i * sigma0 of rbl_set_row_weights) in the
 * place of sigma0: the row-weighted twin of whichever instance rbl_k_sweep_erm runs at that width - same launcher, same
 * num_cu and instance reporting, same NaN presets and guard behind row n.  sigma_i == sigma0 for all i gives
 * rbl_k_sweep_erm's bits.  sigma NULL is RBL_ERR_INVALID. */
int  rbl_k_sweep_erm_w(int storage, int loss, int64_t n, int64_t d, const double* D, const double* w, const double* z_old,
                       const double* lam, const double* sigma /* n */, double rho, double rho_next, int num_cu, int want_v,
                       double* lam_out, double* v, double* z_new, double* q, double* primal2, double* zz, int* instance);
int  rbl_k_sweep_v(int storage, int64_t n, int64_t d, const double* D, const double* w, const double* z, const double* lam,
                   double rho, int num_cu, double* lam_out, double* v, double* primal2, int* instance);
int  rbl_k_sweep_q(int storage, int64_t n, int64_t d, const double* D, const double* c, int num_cu, double* q, int* instance);
int  rbl_k_sweep_v_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* W, const double* Z,
                         const double* LAM, const double* rho, int num_cu, double* LAM_out, double* V, double* primal2,
                         int* instance);
int  rbl_k_sweep_q_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* C, int num_cu, double* Q,
                         int* instance);
/* The plain passes (sweep.hip) and the Gram kernels (gram.hip) on prescribed inputs with a caller-chosen grid: the
 * launchers a solve runs, unchanged, with `num_cu` (1 .. the device's count, else RBL_ERR_INVALID) in the place of the
 * device's CU count and buffers sized by the launchers' own rules for that num_cu.  Host fp64 in and out; D is rounded
 * to `storage`; ld = d rounded up to the storage's row stride.  Outputs over the columns come back at full length ld
 * and are preset to 0xff bytes on the device: the pad [d, ld) is part of what a pass must write (+0.0).
 *   rbl_k_pass_v         v = D w through launch_gemv.  v is preset to NaN with a guard behind row n, as in rbl_k_sweep_*.
 *                        instance (6 ints): 0, LPR lanes per row, P passes (0: w staged in LDS), U, blocks, 1.
 *                        A row wider than the LDS-staged path takes (ld x 8 > 150 KiB) is RBL_ERR_INVALID.
 *   rbl_k_pass_q         q = D^T c through launch_gemvt, its routing to the Q-only pass at 33..512 packets per row
 *                        included.  instance: 0, TPR threads per row, PJ packets per thread, U, row blocks, column tiles -
 *                        or 1, P, R, S, blocks, 0 when the Q-only pass ran (rbl_k_sweep_q tests that one).
 *   rbl_k_pass_colstats  column sums and sums of squares through launch_colstats (RBL_STORE_F32 / F64; F16 is
 *                        RBL_ERR_INVALID); instance as rbl_k_pass_q's first form, at every width.
 *   rbl_k_gram_full      G = D^T D through launch_gram, all ld x ld entries; plan (4 x int64): column tiles, tile pairs,
 *                        row splits, rows per split. */
int  rbl_k_pass_v(int storage, int64_t n, int64_t d, const double* D, const double* w, int num_cu, double* v, int* instance);
int  rbl_k_pass_q(int storage, int64_t n, int64_t d, const double* D, const double* c, int num_cu, double* q_ld,
                  int* instance);
int  rbl_k_pass_colstats(int storage, int64_t n, int64_t d, const double* D, int num_cu, double* sum_ld, double* sumsq_ld,
                         int* instance);
int  rbl_k_gram_full(int storage, int64_t n, int64_t d, const double* D, int num_cu, double* G_ld, int64_t* plan);
/* G = D^T D (MFMA f64) */
int  rbl_k_gram(int storage, int64_t n, int64_t d, const double* D, double* G);
/* the passes of RBL_STORE_CSR on a host CSR matrix that holds D itself (no label sign): int64 indptr (n + 1), int32
 * indices and fp64 values (indptr[n] entries each, canonical rows).  They run the launches a handle runs: the forming
 * kernel, the column-form build, the pass.  q has ld entries (d rounded up to a multiple of 4): the padding is written too. */
int  rbl_k_csr_gemv(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
                    const double* w, double* v);
int  rbl_k_csr_gemvt(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
                     const double* c, double* q);
/* the multi-column sparse passes of the groups (RBL_GROUP_SHARE_SPARSE) through their launchers, on a grid sized for
 * num_cu (1 .. the device's count, else RBL_ERR_INVALID); 1 <= k <= 4, k == 1 is the single-column pass.  W: k x d,
 * V: k x n (row j = D w_j; from a buffer preset to NaN with a guard behind row n that the entry checks); C: k x n,
 * Q: k x ld (row j = D^T c_j, the padding included; Q and the segments' partial sums are preset to 0xff).  lanes_out:
 * the lane group of v = D w (4 .. 64); nseg_out: the segments of q = D^T c.  Either may be NULL. */
int  rbl_k_csr_gemv_multi(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int k,
                          const double* W, int num_cu, double* V, int* lanes_out);
int  rbl_k_csr_gemvt_multi(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int k,
                           const double* C, int num_cu, double* Q, int64_t* nseg_out);
int  rbl_k_csr_gram(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, double* G);
/* rbl_k_csr_gram with the route (0 = the rule's, 2, 3), the grid and the tile width (0 = the plan's) chosen by the
 * caller - launcher arguments like num_cu elsewhere, not switches; G_ld: all ld x ld entries, from a buffer the entry
 * presets to 0xff */
int  rbl_k_csr_gram_route(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
                          int route, int num_cu, int tile_cols, double* G_ld, rbl_gram_report* rep);
/* w-steps in Gram space: lasso / ridge / smoothed-l1 */
int  rbl_k_wstep(int wstep, int64_t d, const double* G, const double* q, double rho, double reg,
                 double smooth_t, const double* w0, double tol, double* w_out, int* iters);
/* the w-step with per-coordinate penalties (rbl_set_penalty) over host buffers: the lasso form when any l1[j] > 0,
 * else CG; *form as rbl_stats.wstep_form reports it (2 active-set kernel, 0 / 1 CG or FISTA) */
int  rbl_k_wstep_pen(int64_t d, const double* G, const double* q, double rho, const double* l1, const double* l2,
                     const double* w0, double tol, double* w_out, int* iters, int* form);
/* The operator w-step of RBL_CREATE_NO_GRAM over host buffers: the CSR arrays hold D itself (n x d, canonical rows, as
 * rbl_k_csr_gemv takes them); both forms are built, L = 1.02 lambda_max(D^T D) comes from the power iteration through the
 * operator as on a handle, then ONE w-step: wstep 2 solves (rho D^T D + reg I) w = rho q by CG, wstep 1 the lasso
 * min 1/2 w'D^T D w - q'w + reg/(2 rho) ||w||_1 by FISTA; with l1 / l2 (d each, either may be NULL) the per-coordinate
 * forms of rbl_set_penalty (reg is then not used).  w_inout: ld = d rounded up to 4 doubles - in: the warm start (the
 * first d are read), out: all ld, the padding as the kernels left it (+0.0).  num_cu sizes the grids of the sparse
 * passes (0: the device's); no bit of the result depends on it.  *status: 1 converged, 0 max_inner reached.
 * RBL_WSTEP_SMOOTH_L1, NULL pointers, n or d < 1 are RBL_ERR_INVALID with a message. */
int  rbl_k_wstep_op(int wstep, int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
                    const double* q, double rho, double reg, const double* l1 /* NULL */, const double* l2 /* NULL */,
                    double tol, int max_inner, int num_cu, double* w_inout, int* iters, int* status);
/* ---- the working-set lasso of RBL_CREATE_WORKING_SET (wstep_ws.hip; src/optim/algorithms.py:190-202, src/util/fast_lasso.py) */
typedef struct rbl_wset_report {
    int32_t slots;        /* slots of the working set in use */
    int32_t support;      /* coefficients != 0 after the last w-step (-1: it left the route) */
    int32_t rounds;       /* solve + scan rounds of the last w-step */
    int32_t pass_pairs;   /* D^T (D w) evaluations - two sparse passes each - of the last w-step */
    int32_t rows_last;    /* rows of the sub-Gram matrix formed in the last w-step */
    int32_t fista_on_gs;  /* 1: a restricted solve of the last w-step fell to FISTA on the sub-Gram matrix */
    int32_t left_route;   /* 1: the last w-step left the route (operator FISTA, wstep_form 4) */
    int32_t form;         /* rbl_stats.wstep_form of the last w-step, 0 = none yet */
    int64_t rows_total;   /* rows formed since the working set was last emptied ... */
    int64_t evictions;    /* ... and slots evicted */
    int64_t bytes;        /* device bytes the working set holds */
} rbl_wset_report;
/* the working set of h; RBL_ERR_STATE on a handle created without RBL_CREATE_WORKING_SET */
int  rbl_wset_info(rbl_solver* h, rbl_wset_report* out);
/* k_ws_gram_rows over host buffers: the CSR arrays hold D (as rbl_k_wstep_op takes them); cols[0 .. ncols) are appended to
 * an empty working set in that order, in calls of split[0], split[1], ... columns (nsplit >= 1, the sum is ncols; NULL:
 * one call) -> Gs_out, 1024 x 1024 doubles, slot a = cols[a].  ncols <= 1024, the columns distinct and in [0, d). */
int  rbl_k_wset_gram(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* cols,
                     int ncols, const int32_t* split, int nsplit, int num_cu, double* Gs_out);
/* k_ws_scan / k_ws_select on prescribed vectors of ld doubles (ld even): g, kappa (per column), q (NULL: zeros), member
 * (ld ints, != 0: in S); columns >= d are never chosen.  cols_out: room for 64; *count the columns chosen (take <= 64). */
int  rbl_k_wset_scan(int64_t ld, int64_t d, const double* g, const double* kappa, const double* q, const int32_t* member, double tol,
                     int take, int32_t* cols_out, int* count);
/* rbl_k_wstep_op's arguments for wstep 1, K right-hand sides Q (K x d) run one after another on ONE workspace as
 * rbl_k_wstep_seq does (step k warm-started from step k - 1, step 0 from w_inout), through run_wstep_ws as a handle
 * created with RBL_CREATE_WORKING_SET runs it.  ws_cap: the slots the working set may use (0 = 1024; a test argument).
 * W_out: K x ld, reports: K. */
int  rbl_k_wstep_ws(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int K,
                    const double* Q, double rho, double reg, const double* l1 /* NULL */, const double* l2 /* NULL */, double tol,
                    int max_inner, int num_cu, int ws_cap, const double* w0 /* NULL = 0 */, double* W_out, rbl_wset_report* reports);
/* K >= 1 w-steps one after another on ONE workspace, as consecutive ADMM iterations run them: step k solves for the
 * right-hand side Q[k] (K x d), warm-started from the w of step k - 1 (step 0 from w0, NULL = 0), through run_wstep
 * unchanged - the batch sizes, the back-off of the nonlinear CG's linear phase, the exchange tags and the uncleared
 * exchange buffers all carry over from step to step.  l1 / l2 (d each, either may be NULL) are per-coordinate penalties
 * as in rbl_k_wstep_pen (wstep 1 or 2 only; reg is then not used).
 *   route        0: as the solver runs with one live handle (the persistent kernels where the width allows them);
 *                1: the batched launches - the workspace has no exchange buffers, the test a second live handle fails too
 *                2: (wstep 2 only) the eigendecomposition ridge: G is decomposed once on the workspace as rbl_gram_finish
 *                   does under RBL_RIDGE_EIG=1 (no environment variable is read here), with its ld <= 2048 rule; where
 *                   the Jacobi converged every step reports form 3 and iters 1, where it did not (or ld > 2048, or with
 *                   l1 / l2) the steps run as under route 0 - the report's form says which
 *   launch_seq0  the workspace's launch counter before the first step (0 .. 0xfffff)
 *   flags        RBL_KW_WANT_GW  ask for G w of the solution (want_Gw);
 *                RBL_KW_W_PREV   let the lasso kernel save its warm start (w_prev_out);
 *                RBL_KW_RHO_DEV  the lasso kernel reads rho on the device (the host passes 1.0 in its place, as the
 *                                speculative w-step does; implies RBL_KW_TWO_CALL, whose second call knows rho);
 *                RBL_KW_TWO_CALL the lasso as run_wstep(fs_pending) followed by finish_wstep_l1
 * Outputs, K rows each: W (K x d); Gw (K x d, optional): the workspace's G w where the step declared it valid (the
 * persistent kernels with RBL_KW_WANT_GW, the lasso kernel when its status is 0), NaN elsewhere; Wprev (K x d, optional):
 * what the lasso kernel saved, NaN where nothing was; reports (K, optional).
 * Every argument is checked before anything is allocated (RBL_ERR_INVALID). */
enum { RBL_KW_WANT_GW = 1, RBL_KW_W_PREV = 2, RBL_KW_RHO_DEV = 4, RBL_KW_TWO_CALL = 8 };
typedef struct rbl_wstep_report {
    int32_t form;           /* rbl_stats.wstep_form: 0 batched launches, 1 one persistent launch, 2 active-set lasso kernel,
                               3 eigendecomposition ridge (route 2) */
    int32_t status;         /* CG / nonlinear CG: 1 converged, 0 iteration cap (the kernel's own word); lasso: fs[0] */
    int32_t iters;          /* as run_wstep / finish_wstep_l1 return them */
    int32_t glds, per, nblocks, lds_bytes;   /* the persistent instance the step launched (G rows in LDS, elements per
                                                thread, blocks, dynamic LDS bytes), 0 when none ran.  form 1 has one; so
                                                has form 0 with status 0 under wstep 3: the nonlinear CG reached its
                                                iteration cap and FISTA finished the step */
    int32_t phase_a;        /* persistent nonlinear CG: linear first phase -1 not tried, 0 dropped, 1 accepted; else -1 */
    int32_t fs[4];          /* lasso kernel: status (0 converged, 1 overflow, 2 cap), outer iterations, steps, support */
    int32_t fell_back;      /* lasso: FISTA took over */
    int32_t gw_valid;       /* Gw[k] holds G w */
    int32_t last_iters, last_fista, ncg_skip, ncg_backoff, launch_seq;   /* the workspace after the step */
    int32_t live_handles;   /* solver handles of this process alive on the device during the step */
} rbl_wstep_report;
int  rbl_k_wstep_seq(int wstep, int64_t d, const double* G, int K, const double* Q, double rho, double reg, double smooth_t,
                     const double* l1, const double* l2, const double* w0, double tol, int max_inner, int route,
                     int launch_seq0, int flags, double* W, double* Gw, double* Wprev, rbl_wstep_report* reports);
/* The one-time Jacobi eigendecomposition behind the eigendecomposition ridge (form 3), on a prescribed symmetric PSD G
 * (d x d host doubles, 1 <= d, round_up(d, 4) <= 2048): G is zero-padded to ld = round_up(d, 4) as rbl_k_wstep_seq pads
 * it and decomposed on a scratch stream.  Outputs (host): Vt_ld (ld x ld, row j = eigenvector j), V_ld (ld x ld, its
 * transpose), lambda_ld (ld), *ld, *sweeps = the Jacobi sweeps run, 0 = not converged within the cap - the solver then
 * keeps the CG, and V_ld / lambda_ld are NaN (only a converged run writes them; Vt_ld holds the last iterate).
 * Every argument is checked before anything is allocated (RBL_ERR_INVALID).  The presence of this symbol is the
 * capability probe (RBL_VERSION is unchanged). */
int  rbl_k_eig(int64_t d, const double* G, double* Vt_ld, double* V_ld, double* lambda_ld, int64_t* ld, int* sweeps);
/* sigma generators (src/optim/objective.py:97-164) */
int  rbl_k_weights(int weight_function, int64_t n, const double* args, int n_args,
                   double* alphas, double* betas);

/* ---- the reference's competitor baselines ---------------------------------------------------
 * SGDmethod (SGD_solver.py:9-96 -> StochasticSubgradientMethod, existing_methods/lerm_main/src/optim/algorithms.py:54-98)
 * and LSVRGmethod (LSVRG_solver.py:9-98 -> LSVRG, algorithms.py:150-253) on the competitor's objective
 * (existing_methods/lerm_main/src/optim/objective.py:41-112).  One call = one epoch.  The index and random-sign
 * streams are the reference's own host generators (torch.randperm / numpy RandomState / numpy.random.choice /
 * torch.rand) and are passed in as data; the Python mirrors SGD_solver.py / LSVRG_solver.py of the package draw
 * them exactly as the reference does.  X: n x d host rows (float64), y01: labels in {0, 1} (the reference maps -1
 * to 0 for both losses, SGD_solver.py:13-14). */
typedef struct rbl_baseline rbl_baseline;
int  rbl_bl_create(int64_t n, int64_t d, const double* X, const double* y01, int loss, int has_lossB, double lossB,
                   double l2_reg, double l1_reg, int device, rbl_baseline** out);
int  rbl_bl_destroy(rbl_baseline* h);
int  rbl_bl_set_w(rbl_baseline* h, const double* w);
int  rbl_bl_get_w(rbl_baseline* h, double* w);
/* StochasticSubgradientMethod.start_epoch + `steps` x step (algorithms.py:80-93): mini-batch s = rows
 * order[s*batch .. (s+1)*batch); alphas_b / betas_b: the `batch`-sample weights (objective.py:72-75;
 * betas_b NULL unless EHRM); rands: one torch.rand(1) per step for the l1 subgradient at 0 (NULL without l1_reg).
 * Every mini-batch is whole: steps * batch > n is RBL_ERR_INVALID, because the reference weights a short last
 * mini-batch of b < batch rows with the b-sample weights (objective.py:72-77), which this call does not carry
 * (SGDmethod never makes one: steps = min(100, n / batch)).  rands == NULL on a handle created with l1_reg != 0 is
 * RBL_ERR_INVALID when steps > 0, here and in rbl_bl_lsvrg_epoch.  A refused call leaves w as it was. */
int  rbl_bl_sgd_epoch(rbl_baseline* h, const int32_t* order, int steps, int batch, const double* alphas_b,
                      const double* betas_b, double lr, const float* rands);
/* LSVRG.start_epoch + `steps` x step (algorithms.py:183-253): alphas / betas are the n-sample weights; samples[s]
 * is a row index (uniform != 0: RandomState.randint) or a rank of the checkpoint's sorted order (uniform == 0:
 * numpy.random.choice(n, p=alphas)) */
int  rbl_bl_lsvrg_epoch(rbl_baseline* h, const double* alphas, const double* betas, const int32_t* samples, int steps,
                        int uniform, double lr, const float* rands);

#ifdef __cplusplus
}
#endif
#endif /* RBL_H */
