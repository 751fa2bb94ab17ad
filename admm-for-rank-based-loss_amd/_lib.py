"""ctypes binding of librbl.so (include/rbl.h).

The HIP library is the product: when it is missing or no GPU is present every compute
call fails loudly (there is no CPU fallback and nothing here imports the test oracle).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librbl.so")

RBL_OK, RBL_ERR_INVALID, RBL_ERR_NO_DEVICE, RBL_ERR_HIP, RBL_ERR_STATE, RBL_ERR_NOMEM = 0, -1, -2, -3, -4, -5
LOSS = {"binary_cross_entropy": 0, "hinge": 1, "squared_hinge": 2}
WEIGHT = {"erm": 0, "extremile": 1, "superquantile": 2, "esrm": 3, "aorr": 4, "aorr_dc": 5, "ehrm": 6}
WSTEP_L1, WSTEP_L2, WSTEP_SMOOTH_L1 = 1, 2, 3
# "csr" (RBL_STORE_CSR): D stays sparse on the device - its entries as float64, so nothing is rounded
STORAGE = {"f32": 0, "float32": 0, "f64": 1, "float64": 1, "fp16": 2, "float16": 2, "csr": 3}
STORE_CSR = 3
_STORAGE_DTYPE = {0: np.float32, 1: np.float64, 2: np.float16, 3: np.float64}
# rbl_set_data_from: element type of the caller's X, where it lives, column scaling, flags
DTYPE_F64, DTYPE_F32, DTYPE_F16 = 0, 1, 2
SOURCE_DTYPE = {np.dtype(np.float64): DTYPE_F64, np.dtype(np.float32): DTYPE_F32, np.dtype(np.float16): DTYPE_F16}
MEM_HOST, MEM_DEVICE = 0, 1
SCALING = {"none": 0, "fit": 1, "apply": 2}
DATA_ONES_COLUMN = 1
GROUP_SHARE_SPARSE = 1          # rbl_group_create_opts: shared multi-column passes on storage "csr"
CREATE_NO_GRAM = 1              # rbl_create_opts: no Gram matrix, the operator w-step (storage "csr")
CREATE_WORKING_SET = 2          # ... and the exact working-set lasso as its l1 w-step (with CREATE_NO_GRAM, wstep l1)
L1_SOLVERS = ("fista", "working_set")
WS_CAP, WS_SELECT = 1024, 64    # csrc/wset_plan.h: slots of the working set, columns one scan adds at most
GRAM_MAX_LD = 16384             # the widest ld of the Gram-space w-step (csrc/rbl_internal.h: RBL_GRAM_MAX_LD)
GRAM_MODES = ("auto", "dense", "none")
# rbl_set_data_csr: the type of indptr and indices
INDEX_I32, INDEX_I64 = 0, 1
INDEX_DTYPE = {np.dtype(np.int32): INDEX_I32, np.dtype(np.int64): INDEX_I64}


def storage_ld(d, storage):
    """Row stride (elements) of the stored matrix: rows are whole 16-byte packets, zero padded - a multiple of 8 elements
    with fp16 storage, of 4 with f32 / f64.  "csr" stores no rows; its vectors of length ld follow the f64 rule."""
    e = 8 if STORAGE[storage] == 2 else 4
    return (int(d) + e - 1) // e * e


def storage_round(X, storage):
    """The matrix the device stores for X, as float64: every entry rounded once (to nearest even) to the storage type.
    The device solves, in fp64 arithmetic, the problem whose data matrix is this one.  A finite entry that does not fit the
    storage type (fp16: |x| >= 65520) is a ValueError, as it is in rbl_set_data - never clipped."""
    X = np.asarray(X, dtype=np.float64)
    dt = _STORAGE_DTYPE[STORAGE[storage]]
    with np.errstate(over="ignore"):
        R = X.astype(dt).astype(np.float64)
    bad = np.isinf(R) & np.isfinite(X)
    if bad.any():
        first = np.argwhere(bad)[0]
        where = ", ".join(str(int(i)) for i in first)
        name = {np.float16: "fp16", np.float32: "f32"}[dt]
        limit = {np.float16: "float16 (|x| >= 65520)", np.float32: "float32"}[dt]
        raise ValueError(f"{name} storage: {int(bad.sum())} finite entries do not fit {limit}, first at index ({where}) "
                         f"(value {float(X[tuple(first)]):g}) - standardise the columns or use storage {'f32' if dt is np.float16 else 'f64'}")
    return R
BUF_M, BUF_Q, BUF_RED, BUF_G, BUF_V, BUF_Z, BUF_LAM, BUF_W, BUF_COLSTATS = range(9)
(BUF_ZD_SKEYS, BUF_ZD_SIDS, BUF_ZD_RKEYS, BUF_ZD_RIDS, BUF_ZD_SMALL, BUF_ZD_BIDS, BUF_ZD_BU, BUF_ZD_ZIDS,
 BUF_ZD_ZU, BUF_ZD_COUNTS) = range(16, 26)
BUF_ZB_HIST, BUF_ZB_TOT, BUF_ZB_PACK = 26, 27, 28
KERNEL_GEMV, KERNEL_GEMVT, KERNEL_SWEEP_ERM = 0, 1, 2
KERNEL_SRC_STATS, KERNEL_SRC_FORM = 3, 4      # the two passes of the last rbl_set_data_from


class RblConfig(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("d", C.c_int64), ("n_total", C.c_int64), ("row_offset", C.c_int64),
        ("loss", C.c_int32), ("weight_function", C.c_int32),
        ("weight_args", C.c_double * 2),
        ("n_weight_args", C.c_int32), ("has_B", C.c_int32),
        ("B", C.c_double),
        ("wstep", C.c_int32),
        ("reg", C.c_double), ("smooth_t", C.c_double), ("rho0", C.c_double), ("tol", C.c_double),
        ("w_tol", C.c_double),
        ("max_iter", C.c_int32), ("storage", C.c_int32), ("device", C.c_int32), ("objective_only", C.c_int32),
    ]


class RblStats(C.Structure):
    _fields_ = [
        ("iter", C.c_int64),
        ("primal", C.c_double), ("dual", C.c_double), ("rho", C.c_double), ("rho_next", C.c_double),
        ("objective", C.c_double),
        ("converged", C.c_int32), ("inner_iters", C.c_int32), ("ehrm_branch", C.c_int32), ("pav_merges", C.c_int32),
        ("ms_z", C.c_float), ("ms_q", C.c_float), ("ms_w", C.c_float), ("ms_v", C.c_float), ("ms_total", C.c_float),
        ("fused", C.c_int32), ("mispredicted", C.c_int32),
        ("fused_v", C.c_int32), ("host_syncs", C.c_int32), ("sort_passes", C.c_int32), ("zband", C.c_int32),
        ("wstep_form", C.c_int32),
    ]


class RblWstepReport(C.Structure):
    """rbl_wstep_report of include/rbl.h: what one step of rbl_k_wstep_seq ran"""
    _fields_ = [
        ("form", C.c_int32), ("status", C.c_int32), ("iters", C.c_int32),
        ("glds", C.c_int32), ("per", C.c_int32), ("nblocks", C.c_int32), ("lds_bytes", C.c_int32),
        ("phase_a", C.c_int32),
        ("fs", C.c_int32 * 4),
        ("fell_back", C.c_int32), ("gw_valid", C.c_int32),
        ("last_iters", C.c_int32), ("last_fista", C.c_int32), ("ncg_skip", C.c_int32), ("ncg_backoff", C.c_int32),
        ("launch_seq", C.c_int32), ("live_handles", C.c_int32),
    ]


class RblGramReport(C.Structure):
    """rbl_gram_report of include/rbl.h: how a Gram matrix was formed"""
    _fields_ = [
        ("route", C.c_int32), ("tile_cols", C.c_int32),
        ("items", C.c_int64), ("batches", C.c_int64),
        ("pair_products", C.c_int64), ("dense_products", C.c_int64), ("transient_bytes", C.c_int64),
        ("ms", C.c_float),
    ]


class RblWsetReport(C.Structure):
    """rbl_wset_report of include/rbl.h: the working set after the last w-step"""
    _fields_ = [
        ("slots", C.c_int32), ("support", C.c_int32), ("rounds", C.c_int32), ("pass_pairs", C.c_int32),
        ("rows_last", C.c_int32), ("fista_on_gs", C.c_int32), ("left_route", C.c_int32), ("form", C.c_int32),
        ("rows_total", C.c_int64), ("evictions", C.c_int64), ("bytes", C.c_int64),
    ]


def _wset_report_dict(r):
    return {name: int(getattr(r, name)) for name, _ in RblWsetReport._fields_}


def _gram_report_dict(r):
    return {name: (float(r.ms) if name == "ms" else int(getattr(r, name))) for name, _ in RblGramReport._fields_}


KW_WANT_GW, KW_W_PREV, KW_RHO_DEV, KW_TWO_CALL = 1, 2, 4, 8


class RblError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librbl error {code}: {msg}")
        self.code = code
        self.msg = msg


_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes): every symbol include/rbl.h declares
SIGNATURES = {
    "rbl_version": (C.c_int, []),
    "rbl_sizeof": (C.c_int, [C.c_int]),
    "rbl_last_error": (C.c_char_p, []),
    "rbl_device_count": (C.c_int, []),
    "rbl_create": (C.c_int, [C.POINTER(RblConfig), C.POINTER(_P)]),
    "rbl_create_opts": (C.c_int, [C.POINTER(RblConfig), C.c_uint32, C.POINTER(_P)]),
    "rbl_destroy": (C.c_int, [_P]),
    "rbl_create_shared": (C.c_int, [C.POINTER(RblConfig), _P, C.POINTER(_P)]),
    "rbl_set_labels": (C.c_int, [_P, _P]),
    "rbl_set_penalty": (C.c_int, [_P, _P, _P]),
    "rbl_get_penalty": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "rbl_set_row_weights": (C.c_int, [_P, _P]),
    "rbl_get_row_weights": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "rbl_decide_multi": (C.c_int, [_P, C.c_int, _P, _P]),
    "rbl_group_create": (C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "rbl_group_create_opts": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.POINTER(_P)]),
    "rbl_group_profile": (C.c_int, [_P, C.c_int]),
    "rbl_group_pass_times": (C.c_int, [_P, _D, _I64]),
    "rbl_group_destroy": (C.c_int, [_P]),
    "rbl_group_step": (C.c_int, [_P, C.c_int, C.POINTER(RblStats)]),
    "rbl_group_solve": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(RblStats), _P, _P, _P, _P, _I64, C.c_int64]),
    "rbl_group_counters": (C.c_int, [_P, C.POINTER(C.c_int), _I64, _I64, _I64]),
    "rbl_set_stream": (C.c_int, [_P, _P]),
    "rbl_set_data": (C.c_int, [_P, _P, _P, C.c_int64]),
    "rbl_set_data_from": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, _P, C.c_int, C.c_int]),
    "rbl_set_data_csr": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "rbl_set_scaling": (C.c_int, [_P, _P, _P]),
    "rbl_get_scaling": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "rbl_set_centering": (C.c_int, [_P, C.c_int]),
    "rbl_get_centering": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rbl_generate_synthetic": (C.c_int, [_P, C.c_uint64, C.c_double, C.c_double]),
    "rbl_synth_local": (C.c_int, [_P, C.c_uint64, C.c_double, C.c_double]),
    "rbl_synth_finish": (C.c_int, [_P]),
    "rbl_get_labels": (C.c_int, [_P, _P]),
    "rbl_gram_local": (C.c_int, [_P]),
    "rbl_gram_finish": (C.c_int, [_P]),
    "rbl_get_D": (C.c_int, [_P, _P]),
    "rbl_get_state": (C.c_int, [_P, _P, _P, _P, _D, _I64, _D]),
    "rbl_set_state": (C.c_int, [_P, _P, _P, _P, _D, _I64, _D]),
    "rbl_get_sigma": (C.c_int, [_P, _P, _P]),
    "rbl_step": (C.c_int, [_P, C.c_int, C.POINTER(RblStats)]),
    "rbl_solve": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(RblStats), _P, _P, _P, _P, _P, C.c_int64]),
    "rbl_finalize_smooth": (C.c_int, [_P]),
    "rbl_objective": (C.c_int, [_P, _P, C.c_int, _D]),
    "rbl_accuracy": (C.c_int, [_P, _P, C.c_double, _D]),
    "rbl_fair_statistics": (C.c_int, [_P, _P, _P, C.c_double, _P]),
    "rbl_phase_m": (C.c_int, [_P]),
    "rbl_phase_z": (C.c_int, [_P, _P]),
    "rbl_phase_z_external": (C.c_int, [_P, _P]),
    "rbl_phase_w_external": (C.c_int, [_P, _P]),
    "rbl_zd_sort_local": (C.c_int, [_P, C.c_int]),
    "rbl_zd_partition": (C.c_int, [_P, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "rbl_zd_prepare": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "rbl_zd_sort_losses": (C.c_int, [_P, C.c_int]),
    "rbl_zd_risk": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "rbl_zd_pav": (C.c_int, [_P, C.c_void_p]),
    "rbl_zd_bounds": (C.c_int, [_P]),
    "rbl_zd_seam_setup": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rbl_zd_seam_propose": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p]),
    "rbl_zd_seam_eval": (C.c_int, [_P, C.c_int, C.c_void_p]),
    "rbl_zd_seam_sums": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "rbl_zd_seam_fill": (C.c_int, [_P, C.c_void_p]),
    "rbl_zd_return_partition": (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    "rbl_zd_scatter": (C.c_int, [_P, C.c_int64]),
    "rbl_zbd_begin": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rbl_zbd_hist": (C.c_int, [_P, C.c_int]),
    "rbl_zbd_scan": (C.c_int, [_P, C.c_int]),
    "rbl_zbd_eval": (C.c_int, [_P, C.c_int]),
    "rbl_zbd_decide": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rbl_zbd_root_passes": (C.c_int, []),
    "rbl_zbd_gather": (C.c_int, [_P, C.c_int]),
    "rbl_zbd_finish": (C.c_int, [_P, C.c_int, C.c_void_p, C.c_int]),
    "rbl_zbd_apply": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rbl_phase_q": (C.c_int, [_P]),
    "rbl_phase_w": (C.c_int, [_P]),
    "rbl_phase_dual": (C.c_int, [_P, C.c_int]),
    "rbl_phase_finish": (C.c_int, [_P, C.POINTER(RblStats)]),
    "rbl_buffer": (C.c_int, [_P, C.c_int, C.POINTER(_P), _I64]),
    "rbl_pending_reduce": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rbl_risk_from_v": (C.c_int, [_P, _P, _D]),
    "rbl_info": (C.c_int, [_P, _I64, C.POINTER(C.c_int), _D]),
    "rbl_kernel_time": (C.c_int, [_P, C.c_int, _D, _I64]),
    "rbl_reset_kernel_times": (C.c_int, [_P]),
    "rbl_kernel_samples": (C.c_int, [_P, C.c_int, _P, C.c_int64, _I64]),
    "rbl_profile_kernels": (C.c_int, [_P, C.c_int]),
    "rbl_profile_sampling": (C.c_int, [_P, C.c_int]),
    "rbl_k_prox": (C.c_int, [C.c_int, C.c_int64, _P, C.c_double, _P, _P]),
    "rbl_k_sort": (C.c_int, [C.c_int64, _P, _P, _P]),
    "rbl_k_sort32": (C.c_int, [C.c_int64, _P, C.c_uint32, _P, _P, C.POINTER(C.c_int)]),
    "rbl_zband_status": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rbl_risk_path": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rbl_k_pav": (C.c_int, [C.c_int, C.c_int64, _P, C.c_double, _P, _P, _I64]),
    "rbl_k_pav_ehrm": (C.c_int, [C.c_int64, _P, _P, C.c_double, C.c_double, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "rbl_k_pav_seq": (C.c_int, [C.c_int, C.c_int64, _P, _P, C.c_double, C.c_double, C.c_int, _P, C.c_int, _P, _P, _P]),
    "rbl_k_gemv": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, _P]),
    "rbl_k_gemvt": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, _P]),
    "rbl_k_gemv_multi": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, _P]),
    "rbl_k_gemvt_multi": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, _P]),
    "rbl_k_sweep_erm": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double,
                                  C.c_int, C.c_int, _P, _P, _P, _P, _D, _D, _P]),
    "rbl_k_sweep_erm_w": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, C.c_double, C.c_double,
                                    C.c_int, C.c_int, _P, _P, _P, _P, _D, _D, _P]),
    "rbl_k_sweep_v": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_double, C.c_int, _P, _P, _D, _P]),
    "rbl_k_sweep_q": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P]),
    "rbl_k_sweep_v_multi": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "rbl_k_sweep_q_multi": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, C.c_int, _P, _P]),
    "rbl_k_pass_v": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P]),
    "rbl_k_pass_q": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P]),
    "rbl_k_pass_colstats": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, C.c_int, _P, _P, _P]),
    "rbl_k_gram_full": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, C.c_int, _P, _P]),
    "rbl_k_gram": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P]),
    "rbl_k_csr_gemv": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    "rbl_k_csr_gemvt": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    "rbl_k_csr_gemv_multi": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, C.c_int, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "rbl_k_csr_gemvt_multi": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, C.c_int, _P, C.c_int, _P, C.POINTER(C.c_int64)]),
    "rbl_k_csr_gram": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "rbl_k_csr_gram_route": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(RblGramReport)]),
    "rbl_gram_info": (C.c_int, [_P, C.POINTER(RblGramReport)]),
    "rbl_csr_gram_route": (C.c_int, [C.c_int64, C.c_int64, C.c_int64]),
    "rbl_k_wstep": (C.c_int, [C.c_int, C.c_int64, _P, _P, C.c_double, C.c_double, C.c_double, _P, C.c_double, _P,
                              C.POINTER(C.c_int)]),
    "rbl_wset_info": (C.c_int, [_P, C.POINTER(RblWsetReport)]),
    "rbl_k_wset_gram": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "rbl_k_wset_scan": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_double, C.c_int, _P, C.POINTER(C.c_int)]),
    "rbl_k_wstep_ws": (C.c_int, [C.c_int64, C.c_int64, _P, _P, _P, C.c_int, _P, C.c_double, C.c_double, _P, _P, C.c_double,
                                 C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(RblWsetReport)]),
    "rbl_k_wstep_op": (C.c_int, [C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_double, C.c_double, _P, _P, C.c_double,
                                C.c_int, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rbl_k_wstep_pen": (C.c_int, [C.c_int64, _P, _P, C.c_double, _P, _P, _P, C.c_double, _P, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)]),
    "rbl_k_wstep_seq": (C.c_int, [C.c_int, C.c_int64, _P, C.c_int, _P, C.c_double, C.c_double, C.c_double, _P, _P, _P,
                                  C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "rbl_k_eig": (C.c_int, [C.c_int64, _P, _P, _P, _P, _I64, C.POINTER(C.c_int)]),
    "rbl_k_weights": (C.c_int, [C.c_int, C.c_int64, _P, C.c_int, _P, _P]),
    "rbl_bl_create": (C.c_int, [C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                C.POINTER(_P)]),
    "rbl_bl_destroy": (C.c_int, [_P]),
    "rbl_bl_set_w": (C.c_int, [_P, _P]),
    "rbl_bl_get_w": (C.c_int, [_P, _P]),
    "rbl_bl_sgd_epoch": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_double, _P]),
    "rbl_bl_lsvrg_epoch": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_double, _P]),
}

_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (same SONAME as /opt/rocm's).  If librbl.so pulls in the system copy first and torch
    initialises its bundled copy later, the process holds two HIP runtimes and torch then
    reports "No HIP GPUs are available" (measured on the MI355X box, tools/diag_hip_runtime.py).
    Loading torch's copy first makes librbl.so resolve to it as well, whichever module is
    imported first.  Set RBL_NO_TORCH_HIP_PRELOAD=1 to use the system runtime."""
    if os.environ.get("RBL_NO_TORCH_HIP_PRELOAD") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass    # without torch the system runtime is the only one: nothing to reconcile


def load():
    """Load librbl.so; raises (never falls back) when the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _preload_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for which, cls in ((0, RblConfig), (1, RblStats), (2, RblWstepReport), (3, RblGramReport)):
            if lib.rbl_sizeof(which) != C.sizeof(cls):
                raise ImportError(f"{LIB_PATH}: sizeof({cls.__name__}) is {lib.rbl_sizeof(which)} in the library and "
                                  f"{C.sizeof(cls)} in this binding (include/rbl.h and _lib.py out of step: rebuild)")
        _lib = lib
    return _lib


def last_error():
    return load().rbl_last_error().decode("utf-8", "replace")


def check(code):
    if code != RBL_OK:
        msg = last_error()
        if code == RBL_ERR_INVALID:
            raise ValueError(msg)
        raise RblError(code, msg)


def ptr(a):
    """void* of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def device_count():
    return load().rbl_device_count()


# ----------------------------------------------------------- kernel-level wrappers (tests)
def k_prox(loss, sigma, rho, m):
    sigma, m = f64(sigma).reshape(-1), f64(m).reshape(-1)
    out = np.empty_like(m)
    check(load().rbl_k_prox(LOSS[loss], m.size, ptr(sigma), float(rho), ptr(m), ptr(out)))
    return out


def k_sort(keys):
    keys = f64(keys).reshape(-1)
    out = np.empty_like(keys)
    perm = np.empty(keys.size, dtype=np.uint32)
    check(load().rbl_k_sort(keys.size, ptr(keys), ptr(out), ptr(perm)))
    return out, perm


def k_sort32(m, idx_off=0):
    """The z-step's sort with 32-bit keys (include/rbl.h: rbl_k_sort32).  Returns (m_sorted, ids, flag): ids =
    idx_off + row, in (m, row) order; flag = 1: a run of more than 32 equal keys - m_sorted and ids are meaningless."""
    m = f64(m).reshape(-1)
    if not 0 <= int(idx_off) <= (1 << 32) - m.size:
        raise ValueError(f"idx_off must be in [0, 2^32 - n], got {idx_off}")
    out = np.empty_like(m)
    ids = np.empty(m.size, dtype=np.uint32)
    flag = C.c_int(0)
    check(load().rbl_k_sort32(m.size, ptr(m), int(idx_off), ptr(out), ptr(ids), C.byref(flag)))
    return out, ids, flag.value


def k_pav(loss, sigma, rho, m_sorted):
    sigma, m = f64(sigma).reshape(-1), f64(m_sorted).reshape(-1)
    out = np.empty_like(m)
    nm = C.c_int64(0)
    check(load().rbl_k_pav(LOSS[loss], m.size, ptr(sigma), float(rho), ptr(m), ptr(out), C.byref(nm)))
    return out, nm.value


def k_pav_ehrm(sigma_a, sigma_b, B, rho, m_sorted, branch=-1):
    sa, sb, m = f64(sigma_a).reshape(-1), f64(sigma_b).reshape(-1), f64(m_sorted).reshape(-1)
    out = np.empty_like(m)
    br = C.c_int(-1)
    check(load().rbl_k_pav_ehrm(m.size, ptr(sa), ptr(sb), float(B), float(rho), ptr(m), int(branch), ptr(out),
                                C.byref(br)))
    return out, br.value


PAV_UPPER = {"persist": 1, "two_launch": 2}


def k_pav_seq(loss, sigma, rho, m_seq, upper, sigma_b=None, B=0.0):
    """len(m_seq) PAV solves on one workspace (the upper seams' hints, the barrier parity and the EHRM branch carry
    over).  upper: "persist" or "two_launch".  sigma_b: EHRM (BCE).  Returns (u, branch, counters): u (K, n) after the
    EHRM clip, branch (K,) (-1 unless EHRM), counters (K, 4) uint32 = merges, dirty-level mask, long fills, status."""
    sa = f64(sigma).reshape(-1)
    ms = f64(m_seq)
    ms = np.ascontiguousarray(ms.reshape(-1, sa.size))
    K, n = ms.shape
    sb = None if sigma_b is None else f64(sigma_b).reshape(-1)
    out = np.empty((K, n))
    br = np.full(K, -1, dtype=np.int32)
    cnt = np.zeros((K, 4), dtype=np.uint32)
    check(load().rbl_k_pav_seq(LOSS[loss], n, ptr(sa), ptr(sb), float(B), float(rho), K, ptr(ms), PAV_UPPER[upper],
                               ptr(out), ptr(br), ptr(cnt)))
    return out, br, cnt


def k_gemv(D, w, storage="f32"):
    D, w = f64(D), f64(w).reshape(-1)
    v = np.empty(D.shape[0])
    check(load().rbl_k_gemv(STORAGE[storage], D.shape[0], D.shape[1], ptr(D), ptr(w), ptr(v)))
    return v


def k_gemvt(D, c, storage="f32"):
    D, c = f64(D), f64(c).reshape(-1)
    q = np.empty(D.shape[1])
    check(load().rbl_k_gemvt(STORAGE[storage], D.shape[0], D.shape[1], ptr(D), ptr(c), ptr(q)))
    return q


def k_gemv_multi(D, W, storage="f32"):
    """V = D [w_1 .. w_k] through the multi-column pass; W: (k, d) -> V: (k, n)"""
    D, W = f64(D), f64(W)
    W = np.ascontiguousarray(W.reshape(-1, D.shape[1]))
    V = np.empty((W.shape[0], D.shape[0]))
    check(load().rbl_k_gemv_multi(STORAGE[storage], D.shape[0], D.shape[1], W.shape[0], ptr(D), ptr(W), ptr(V)))
    return V


def k_gemvt_multi(D, Cm, storage="f32"):
    """Q = D^T [c_1 .. c_k] through the multi-column pass; Cm: (k, n) -> Q: (k, d)"""
    D, Cm = f64(D), f64(Cm)
    Cm = np.ascontiguousarray(Cm.reshape(-1, D.shape[0]))
    Q = np.empty((Cm.shape[0], D.shape[1]))
    check(load().rbl_k_gemvt_multi(STORAGE[storage], D.shape[0], D.shape[1], Cm.shape[0], ptr(D), ptr(Cm), ptr(Q)))
    return Q


MULTI_KMAX = 4
SWEEP_KIND = {0: "wave", 1: "wide"}


def _instance(a):
    """(kind, P | PT, R, S, blocks) of the kernel instance a rbl_k_sweep_* call ran"""
    return (SWEEP_KIND[int(a[0])], int(a[1]), int(a[2]), int(a[3]), int(a[4]))


def k_sweep_erm(D, w, z_old, lam, sigma0, rho, rho_next, loss, storage="f32", num_cu=1, want_v=True):
    """The single-sweep pass on prescribed inputs with the grid of `num_cu` compute units (include/rbl.h:
    rbl_k_sweep_erm).  Returns a dict: lam, v (all NaN when want_v is False), z, q, primal2, zz, instance."""
    D, w, z_old, lam = f64(D), f64(w).reshape(-1), f64(z_old).reshape(-1), f64(lam).reshape(-1)
    n, d = D.shape
    lam_out, v, z_new, q = np.empty(n), np.empty(n), np.empty(n), np.empty(d)
    p2, zz = C.c_double(0.0), C.c_double(0.0)
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_erm(STORAGE[storage], LOSS[loss], n, d, ptr(D), ptr(w), ptr(z_old), ptr(lam), float(sigma0),
                                 float(rho), float(rho_next), int(num_cu), 1 if want_v else 0, ptr(lam_out), ptr(v),
                                 ptr(z_new), ptr(q), C.byref(p2), C.byref(zz), ptr(inst)))
    return dict(lam=lam_out, v=v, z=z_new, q=q, primal2=p2.value, zz=zz.value, instance=_instance(inst))


def k_sweep_erm_w(D, w, z_old, lam, sigma, rho, rho_next, loss, storage="f32", num_cu=1, want_v=True):
    """k_sweep_erm with one sigma per row (n values) in the place of sigma0: the row-weighted twins (include/rbl.h:
    rbl_k_sweep_erm_w).  Same dict."""
    D, w, z_old, lam = f64(D), f64(w).reshape(-1), f64(z_old).reshape(-1), f64(lam).reshape(-1)
    n, d = D.shape
    sigma = f64(sigma).reshape(-1)
    if sigma.shape[0] != n:
        raise ValueError(f"k_sweep_erm_w: sigma has {sigma.shape[0]} entries, D has {n} rows")
    lam_out, v, z_new, q = np.empty(n), np.empty(n), np.empty(n), np.empty(d)
    p2, zz = C.c_double(0.0), C.c_double(0.0)
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_erm_w(STORAGE[storage], LOSS[loss], n, d, ptr(D), ptr(w), ptr(z_old), ptr(lam), ptr(sigma),
                                   float(rho), float(rho_next), int(num_cu), 1 if want_v else 0, ptr(lam_out), ptr(v),
                                   ptr(z_new), ptr(q), C.byref(p2), C.byref(zz), ptr(inst)))
    return dict(lam=lam_out, v=v, z=z_new, q=q, primal2=p2.value, zz=zz.value, instance=_instance(inst))


def k_sweep_v(D, w, z, lam, rho, storage="f32", num_cu=1):
    """The V-only pass: v = D w, lam + rho (z - v), sum (z - v)^2 (include/rbl.h: rbl_k_sweep_v)"""
    D, w, z, lam = f64(D), f64(w).reshape(-1), f64(z).reshape(-1), f64(lam).reshape(-1)
    n, d = D.shape
    lam_out, v = np.empty(n), np.empty(n)
    p2 = C.c_double(0.0)
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_v(STORAGE[storage], n, d, ptr(D), ptr(w), ptr(z), ptr(lam), float(rho), int(num_cu),
                               ptr(lam_out), ptr(v), C.byref(p2), ptr(inst)))
    return dict(lam=lam_out, v=v, primal2=p2.value, instance=_instance(inst))


def k_sweep_q(D, c, storage="f32", num_cu=1):
    """q = D^T c through the Q-only pass, its widths only (include/rbl.h: rbl_k_sweep_q)"""
    D, c = f64(D), f64(c).reshape(-1)
    n, d = D.shape
    q = np.empty(d)
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_q(STORAGE[storage], n, d, ptr(D), ptr(c), int(num_cu), ptr(q), ptr(inst)))
    return dict(q=q, instance=_instance(inst))


def k_sweep_v_multi(D, W, Z, LAM, rho, storage="f32", num_cu=1):
    """k = 1..4 columns of the V pass with the lambda update in one launch; W: (k, d), Z, LAM: (k, n), rho: (k,).
    lam and v come back as (4, n): the rows behind k are buffers of the entry point that no launch was told about; they
    stay NaN unless a column was written past its n rows (include/rbl.h)."""
    D, W = f64(D), f64(W)
    n, d = D.shape
    W = np.ascontiguousarray(W.reshape(-1, d))
    k = W.shape[0]
    Z, LAM, rho = f64(Z).reshape(k, n), f64(LAM).reshape(k, n), f64(rho).reshape(k)
    lam_out, V = np.empty((MULTI_KMAX, n)), np.empty((MULTI_KMAX, n))
    p2 = np.zeros(k)
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_v_multi(STORAGE[storage], n, d, k, ptr(D), ptr(W), ptr(Z), ptr(LAM), ptr(rho), int(num_cu),
                                     ptr(lam_out), ptr(V), ptr(p2), ptr(inst)))
    return dict(lam=lam_out, v=V, primal2=p2, instance=_instance(inst))


def k_sweep_q_multi(D, Cm, storage="f32", num_cu=1):
    """Q = D^T [c_1 .. c_k] in one launch of the multi-column Q pass, k = 1..4; Cm: (k, n) -> q: (k, d)"""
    D, Cm = f64(D), f64(Cm)
    n, d = D.shape
    Cm = np.ascontiguousarray(Cm.reshape(-1, n))
    k = Cm.shape[0]
    Q = np.empty((k, d))
    inst = np.zeros(5, dtype=np.int32)
    check(load().rbl_k_sweep_q_multi(STORAGE[storage], n, d, k, ptr(D), ptr(Cm), int(num_cu), ptr(Q), ptr(inst)))
    return dict(q=Q, instance=_instance(inst))


def _pass_instance(a):
    """what a rbl_k_pass_* call reports: ("gemv", LPR, P, U, blocks), ("gemvt", TPR, PJ, U, row blocks, column tiles) or,
    where launch_gemvt handed the pass to the Q-only kernel, ("sweep_q", P, R, S, blocks)"""
    a = [int(x) for x in a]
    if a[0] == 1:
        return ("sweep_q", a[1], a[2], a[3], a[4])
    return tuple(a[1:])


def k_pass_v(D, w, storage="f32", num_cu=1):
    """v = D w through launch_gemv with the grid of `num_cu` compute units (include/rbl.h: rbl_k_pass_v); rows the pass
    did not write come back NaN.  Returns a dict: v, instance = (LPR, P, U, blocks)."""
    D, w = f64(D), f64(w).reshape(-1)
    n, d = D.shape
    v = np.empty(n)
    inst = np.zeros(6, dtype=np.int32)
    check(load().rbl_k_pass_v(STORAGE[storage], n, d, ptr(D), ptr(w), int(num_cu), ptr(v), ptr(inst)))
    return dict(v=v, instance=_pass_instance(inst)[:4])


def k_pass_q(D, c, storage="f32", num_cu=1):
    """q = D^T c through launch_gemvt; q has storage_ld(d) entries, the pad included (rbl_k_pass_q).  instance =
    (TPR, PJ, U, row blocks, column tiles), or ("sweep_q", P, R, S, blocks) at the widths of the Q-only pass."""
    D, c = f64(D), f64(c).reshape(-1)
    n, d = D.shape
    q = np.empty(storage_ld(d, storage))
    inst = np.zeros(6, dtype=np.int32)
    check(load().rbl_k_pass_q(STORAGE[storage], n, d, ptr(D), ptr(c), int(num_cu), ptr(q), ptr(inst)))
    return dict(q=q, instance=_pass_instance(inst))


def k_pass_colstats(D, storage="f32", num_cu=1):
    """column sums and sums of squares through launch_colstats, ld entries each (rbl_k_pass_colstats)"""
    D = f64(D)
    n, d = D.shape
    ld = storage_ld(d, storage)
    s1, s2 = np.empty(ld), np.empty(ld)
    inst = np.zeros(6, dtype=np.int32)
    check(load().rbl_k_pass_colstats(STORAGE[storage], n, d, ptr(D), int(num_cu), ptr(s1), ptr(s2), ptr(inst)))
    return dict(sum=s1, sumsq=s2, instance=_pass_instance(inst))


def k_gram_full(D, storage="f32", num_cu=1):
    """G = D^T D through launch_gram, all ld x ld entries; plan = (ntiles, npairs, ksplit, rows_per_split)"""
    D = f64(D)
    n, d = D.shape
    ld = storage_ld(d, storage)
    G = np.empty((ld, ld))
    plan = np.zeros(4, dtype=np.int64)
    check(load().rbl_k_gram_full(STORAGE[storage], n, d, ptr(D), int(num_cu), ptr(G), ptr(plan)))
    return dict(G=G, plan=tuple(int(x) for x in plan))


def k_gram(D, storage="f32"):
    D = f64(D)
    G = np.empty((D.shape[1], D.shape[1]))
    check(load().rbl_k_gram(STORAGE[storage], D.shape[0], D.shape[1], ptr(D), ptr(G)))
    return G


def _csr_arrays(A):
    """(n, d, indptr int64, indices int32, values float64) of a canonical scipy.sparse CSR matrix holding D itself"""
    n, d = A.shape
    return (n, d, np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float64))


def k_csr_gemv(A, w):
    """v = A w through the sparse pass of storage "csr" (A: canonical scipy.sparse CSR, explicit zeros kept)"""
    n, d, ip, ix, va = _csr_arrays(A)
    w = f64(w).reshape(-1)
    v = np.empty(n)
    check(load().rbl_k_csr_gemv(n, d, ptr(ip), ptr(ix), ptr(va), ptr(w), ptr(v)))
    return v


def k_csr_gemvt(A, c):
    """q = A^T c through the column form of storage "csr"; q has storage_ld(d, "csr") entries, the padding included"""
    n, d, ip, ix, va = _csr_arrays(A)
    c = f64(c).reshape(-1)
    q = np.empty(storage_ld(d, "csr"))
    check(load().rbl_k_csr_gemvt(n, d, ptr(ip), ptr(ix), ptr(va), ptr(c), ptr(q)))
    return q


def k_csr_gemv_multi(A, W, num_cu=1):
    """(V, lanes): row j of V = A w_j for the k <= 4 rows of W (k x d) through the groups' multi-column sparse pass on a
    grid sized for num_cu; lanes: the lane group of the pass"""
    n, d, ip, ix, va = _csr_arrays(A)
    W = f64(W).reshape(-1, d)
    V = np.empty((W.shape[0], n))
    lanes = C.c_int(0)
    check(load().rbl_k_csr_gemv_multi(n, d, ptr(ip), ptr(ix), ptr(va), W.shape[0], ptr(W), int(num_cu), ptr(V), C.byref(lanes)))
    return V, lanes.value


def k_csr_gemvt_multi(A, Cm, num_cu=1):
    """(Q, nseg): row j of Q = A^T c_j (storage_ld(d, "csr") entries, the padding included) for the k <= 4 rows of Cm
    (k x n) through the groups' multi-column sparse pass; nseg: the segments of the column form"""
    n, d, ip, ix, va = _csr_arrays(A)
    Cm = f64(Cm).reshape(-1, n)
    Q = np.empty((Cm.shape[0], storage_ld(d, "csr")))
    nseg = C.c_int64(0)
    check(load().rbl_k_csr_gemvt_multi(n, d, ptr(ip), ptr(ix), ptr(va), Cm.shape[0], ptr(Cm), int(num_cu), ptr(Q), C.byref(nseg)))
    return Q, nseg.value


def k_csr_gram(A):
    """G = A^T A by the route the rule of storage "csr" picks (csr_gram_route): from the entries, or row chunks expanded
    through the fp64 MFMA kernel"""
    n, d, ip, ix, va = _csr_arrays(A)
    G = np.empty((d, d))
    check(load().rbl_k_csr_gram(n, d, ptr(ip), ptr(ix), ptr(va), ptr(G)))
    return G


def k_csr_gram_route(A, route=0, num_cu=0, tile_cols=0):
    """(G_ld, report): G = A^T A, all ld x ld entries, by route 0 (the rule's), 2 (dense expansion) or 3 (from the
    entries) on a grid sized for num_cu (0: the device's) with tile_cols columns per accumulator tile (0: the plan's);
    report: the fields of rbl_gram_report"""
    n, d, ip, ix, va = _csr_arrays(A)
    ld = storage_ld(d, "csr")
    G = np.empty((ld, ld))
    rep = RblGramReport()
    check(load().rbl_k_csr_gram_route(n, d, ptr(ip), ptr(ix), ptr(va), int(route), int(num_cu), int(tile_cols), ptr(G), C.byref(rep)))
    return G, _gram_report_dict(rep)


def csr_gram_route(n, ld, pair_products):
    """the rule between the two Gram routes of storage "csr": 2 (dense expansion) or 3 (from the entries); no device"""
    return int(load().rbl_csr_gram_route(int(n), int(ld), int(pair_products)))


def k_wstep(wstep, G, q, rho, reg, w0=None, smooth_t=1.0, tol=1e-13):
    G, q = f64(G), f64(q).reshape(-1)
    d = q.size
    w0 = f64(w0).reshape(-1) if w0 is not None else np.zeros(d)
    out = np.empty(d)
    it = C.c_int(0)
    check(load().rbl_k_wstep(int(wstep), d, ptr(G), ptr(q), float(rho), float(reg), float(smooth_t), ptr(w0),
                             float(tol), ptr(out), C.byref(it)))
    return out, it.value


def k_wstep_pen(G, q, rho, l1=None, l2=None, w0=None, tol=1e-13):
    """The w-step with per-coordinate penalties; returns (w, iterations, form)."""
    G, q = f64(G), f64(q).reshape(-1)
    d = q.size
    l1 = None if l1 is None else f64(np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,)))
    l2 = None if l2 is None else f64(np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,)))
    w0 = f64(w0).reshape(-1) if w0 is not None else np.zeros(d)
    out = np.empty(d)
    it, form = C.c_int(0), C.c_int(0)
    check(load().rbl_k_wstep_pen(d, ptr(G), ptr(q), float(rho), ptr(l1), ptr(l2), ptr(w0), float(tol), ptr(out),
                                 C.byref(it), C.byref(form)))
    return out, it.value, form.value


def k_wstep_op(wstep, A, q, rho, reg=0.0, l1=None, l2=None, w0=None, tol=1e-13, max_inner=100000, num_cu=0):
    """One operator w-step (include/rbl.h: rbl_k_wstep_op) on the canonical scipy.sparse CSR matrix A = D; returns
    (w of storage_ld(d, "csr") entries - the padding included -, iterations, status: 1 converged / 0 cap reached)."""
    n, d, ip, ix, va = _csr_arrays(A)
    q = f64(q).reshape(-1)
    if q.size != d:
        raise ValueError(f"q has {q.size} entries for {d} columns")
    l1 = None if l1 is None else f64(np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,)))
    l2 = None if l2 is None else f64(np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,)))
    w = np.zeros(storage_ld(d, "csr"))
    if w0 is not None:
        w[:d] = f64(w0).reshape(-1)
    it, status = C.c_int(0), C.c_int(0)
    check(load().rbl_k_wstep_op(int(wstep), n, d, ptr(ip), ptr(ix), ptr(va), ptr(q), float(rho), float(reg), ptr(l1), ptr(l2),
                                float(tol), int(max_inner), int(num_cu), ptr(w), C.byref(it), C.byref(status)))
    return w, it.value, status.value


def k_wset_gram(A, cols, split=None, num_cu=0):
    """The working set's sub-Gram matrix (include/rbl.h: rbl_k_wset_gram): the columns ``cols`` of the canonical
    scipy.sparse CSR matrix A appended in that order - in calls of split[0], split[1], ... columns - -> Gs, WS_CAP x WS_CAP
    (slot a = cols[a]; the unused slots zero)"""
    n, d, ip, ix, va = _csr_arrays(A)
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    sp_ = None if split is None else np.ascontiguousarray(split, dtype=np.int32).reshape(-1)
    Gs = np.empty((WS_CAP, WS_CAP))
    check(load().rbl_k_wset_gram(n, d, ptr(ip), ptr(ix), ptr(va), ptr(cols), int(cols.size), ptr(sp_),
                                 0 if sp_ is None else int(sp_.size), int(num_cu), ptr(Gs)))
    return Gs


def k_wset_scan(g, kappa, member, d=None, q=None, tol=1e-13, take=WS_SELECT):
    """The scan's choice on prescribed vectors (include/rbl.h: rbl_k_wset_scan): g, kappa, member of ld entries (ld even),
    the columns >= d never chosen -> the list of chosen columns, in the order they are chosen"""
    g, kappa = f64(g).reshape(-1), f64(kappa).reshape(-1)
    ld = g.size
    member = np.ascontiguousarray(member, dtype=np.int32).reshape(-1)
    q = None if q is None else f64(q).reshape(-1)
    if kappa.size != ld or member.size != ld or (q is not None and q.size != ld):
        raise ValueError(f"g has {ld} entries; kappa, member and q must have as many")
    out, cnt = np.zeros(WS_SELECT, dtype=np.int32), C.c_int(0)
    check(load().rbl_k_wset_scan(ld, ld if d is None else int(d), ptr(g), ptr(kappa), ptr(q), ptr(member), float(tol), int(take),
                                 ptr(out), C.byref(cnt)))
    return out[:cnt.value].tolist()


def k_wstep_ws(A, Q, rho, reg=0.0, l1=None, l2=None, w0=None, tol=1e-13, max_inner=100000, num_cu=0, ws_cap=0):
    """K working-set w-steps one after another on one workspace (include/rbl.h: rbl_k_wstep_ws) on the canonical
    scipy.sparse CSR matrix A = D; Q: (K, d) or (d,).  Returns (W of shape (K, ld) - the padding included -, the K reports
    as dicts of rbl_wset_report's fields)."""
    n, d, ip, ix, va = _csr_arrays(A)
    Q = f64(np.atleast_2d(Q))
    if Q.shape[1] != d:
        raise ValueError(f"Q has {Q.shape[1]} columns for {d} columns of A")
    K = Q.shape[0]
    l1 = None if l1 is None else f64(np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,)))
    l2 = None if l2 is None else f64(np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,)))
    w0 = None if w0 is None else f64(w0).reshape(-1)
    if w0 is not None and w0.size != d:
        raise ValueError(f"w0 has {w0.size} entries for {d} columns")
    W = np.zeros((K, storage_ld(d, "csr")))
    reps = (RblWsetReport * K)()
    check(load().rbl_k_wstep_ws(n, d, ptr(ip), ptr(ix), ptr(va), K, ptr(Q), float(rho), float(reg), ptr(l1), ptr(l2), float(tol),
                                int(max_inner), int(num_cu), int(ws_cap), ptr(w0), ptr(W), reps))
    return W, [_wset_report_dict(r) for r in reps]


def k_wstep_seq(wstep, G, Q, rho, reg, w0=None, smooth_t=1.0, tol=1e-13, max_inner=100000, l1=None, l2=None, route=0,
                launch_seq0=0, want_Gw=False, w_prev=False, rho_dev=False, two_call=False):
    """K w-steps one after another on one workspace, each warm-started from the previous w (include/rbl.h:
    rbl_k_wstep_seq).  Q: (K, d) or (d,).  Returns dict(w (K, d), Gw (K, d; NaN rows where the step left no valid G w),
    w_prev (K, d; NaN where nothing was saved), reports: K dicts of the fields of rbl_wstep_report)."""
    G = f64(G)
    d = G.shape[0]
    Q = np.ascontiguousarray(f64(Q).reshape(-1, d))
    K = Q.shape[0]
    l1 = None if l1 is None else f64(np.broadcast_to(np.asarray(l1, dtype=np.float64), (d,)))
    l2 = None if l2 is None else f64(np.broadcast_to(np.asarray(l2, dtype=np.float64), (d,)))
    w0 = None if w0 is None else f64(w0).reshape(-1)
    flags = (KW_WANT_GW if want_Gw else 0) | (KW_W_PREV if w_prev else 0) | (KW_RHO_DEV if rho_dev else 0) | \
            (KW_TWO_CALL if two_call else 0)
    W, Gw, Wp = np.empty((K, d)), np.empty((K, d)), np.empty((K, d))
    rep = (RblWstepReport * K)()
    check(load().rbl_k_wstep_seq(int(wstep), d, ptr(G), K, ptr(Q), float(rho), float(reg), float(smooth_t), ptr(l1), ptr(l2),
                                 ptr(w0), float(tol), int(max_inner), int(route), int(launch_seq0), flags, ptr(W), ptr(Gw),
                                 ptr(Wp), C.cast(rep, C.c_void_p)))
    reports = [{name: (list(getattr(r, name)) if name == "fs" else int(getattr(r, name))) for name, _ in RblWstepReport._fields_}
               for r in rep]
    return dict(w=W, Gw=Gw, w_prev=Wp, reports=reports)


def k_eig(G):
    """The one-time Jacobi eigendecomposition of the eigendecomposition ridge on a prescribed G (include/rbl.h:
    rbl_k_eig).  Returns dict(Vt (ld x ld, rows = eigenvectors), V (its transpose), lam (ld), ld, sweeps; 0 sweeps = not
    converged: V and lam are then NaN)."""
    G = f64(G)
    d = G.shape[0]
    if G.ndim != 2 or G.shape[1] != d:
        raise ValueError(f"k_eig: G must be square, got shape {G.shape}")
    n = (max(d, 1) + 3) // 4 * 4
    Vt, V, lam = np.empty((n, n)), np.empty((n, n)), np.empty(n)
    ld, sweeps = C.c_int64(0), C.c_int(0)
    check(load().rbl_k_eig(d, ptr(G), ptr(Vt), ptr(V), ptr(lam), C.byref(ld), C.byref(sweeps)))
    assert ld.value == n, (ld.value, n)
    return dict(Vt=Vt, V=V, lam=lam, ld=int(ld.value), sweeps=int(sweeps.value))


def k_weights(weight_function, n, args=None):
    if weight_function not in WEIGHT:
        raise ValueError(
            f"Unrecognized framework '{weight_function}'! Options: ['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']")
    a = np.empty(n)
    b = np.empty(n)
    arr = f64(list(args)) if args is not None else None
    check(load().rbl_k_weights(WEIGHT[weight_function], n, ptr(arr), 0 if arr is None else arr.size, ptr(a), ptr(b)))
    return a, b
