// api.hip - the C ABI of librbl.so (include/rbl.h), first unit: error state, the solver handle's life (create, shared
// create, destroy), its workspaces, state and buffers in and out, the profiling getters.  Host code only orchestrates:
// every arithmetic step runs in a HIP kernel; there is no CPU fallback.  The other units: api_data.hip (data path),
// api_iter.hip (the ADMM iteration), api_dist.hip (distributed z-step), api_group.hip (groups), api_kernels.hip
// (kernel-level entry points of the parity tests).
#include "api_internal.h"

// ------------------------------------------------------------------------- error state
static thread_local std::string g_err;

void rbl_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// -------------------------------------------------------------------------------- handle
// live handles per device: a persistent w-step kernel needs all its blocks resident at once (one per CU: its G rows
// fill the LDS), which only holds while no second such kernel of this process can occupy CUs beside it
static std::atomic<int> g_live[64];
int rbl_live_handles(int device) { return device >= 0 && device < 64 ? g_live[device].load(std::memory_order_relaxed) : 2; }

thread_local int g_host_syncs = 0;   // one solver handle per host thread (include/rbl.h); declared in api_internal.h
void rbl_note_host_sync() { ++g_host_syncs; }

void rbl_spin_wait(const volatile int* word, int sentinel, hipStream_t stream) {
    ++g_host_syncs;
    // No event behind the kernel: an event record costs ~5 us of stream time on this device and
    // the iteration has none left in its steady state.  A launch that failed never writes the
    // word, so after a generous spin the stream itself is waited for (then the word is final).
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned i = 1;; ++i) {
        if (*word != sentinel) return;
        if ((i & 0xffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            (void)hipStreamSynchronize(stream);
            return;
        }
        __builtin_ia32_pause();
    }
}

// RBL_NO_FUSE=1 (tests, comparisons): the two-pass iteration with plain passes - no single-sweep erm pass, no fused V pass
static bool no_fuse() {
    const char* nf = getenv("RBL_NO_FUSE");
    return nf && nf[0] == '1';
}

// The single-sweep erm pass: erm problems at the widths it has instances for.  The sign of a handle's own labels is not
// part of its in-pass prox, so such a handle runs the two-pass iteration.
bool single_sweep_allowed(const rbl_solver* h) {
    return !h->rs && !h->sorted_path && !no_fuse() && sweep_erm_supported(h->storage, h->ld);
}

int alloc_sort(DevArena& mem, SortWorkspace& sw, int64_t n, bool with_vals, hipStream_t s) {
    RBL_TRY(mem.alloc(&sw.keys[0], (size_t)n));
    RBL_TRY(mem.alloc(&sw.keys[1], (size_t)n));
    if (with_vals) {
        RBL_TRY(mem.alloc(&sw.vals[0], (size_t)n));
        RBL_TRY(mem.alloc(&sw.vals[1], (size_t)n));
    }
    RBL_TRY(mem.alloc((unsigned char**)&sw.spine, sort_spine_bytes()));
    RBL_TRY(mem.alloc(&sw.bin_total, 256));
    RBL_TRY(mem.alloc(&sw.bin_base, 256));
    RBL_TRY(mem.alloc((unsigned char**)&sw.ghist, sort_ghist_bytes()));
    RBL_HIP(hipMemsetAsync(sw.ghist, 0, sort_ghist_bytes(), s));
    return RBL_OK;
}

int check_device(int* count_out) {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0) {
        (void)hipGetLastError();
        rbl_set_error("no HIP device available (librbl has no CPU fallback)");
        return RBL_ERR_NO_DEVICE;
    }
    if (count_out) *count_out = cnt;
    return RBL_OK;
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

int alloc_prefix(DevArena& mem, PrefixBufs& p, int64_t n) {
    const int64_t nc = pav_num_chunks(n);
    RBL_TRY(mem.alloc(&p.locx, (size_t)n + 1));
    RBL_TRY(mem.alloc(&p.chunk, (size_t)nc));
    RBL_TRY(mem.alloc(&p.cph, (size_t)nc));
    RBL_TRY(mem.alloc(&p.cpl, (size_t)nc));
    return RBL_OK;
}

int alloc_pav(DevArena& mem, PavWorkspace& pw, int64_t n, hipStream_t s) {
    RBL_TRY(mem.alloc(&pw.ms, (size_t)n));
    RBL_TRY(mem.alloc(&pw.u, (size_t)n));
    RBL_TRY(alloc_prefix(mem, pw.pm, n));
    RBL_TRY(mem.alloc(&pw.recs, (size_t)pav_num_recs(n)));
    RBL_HIP(hipMemsetAsync(pw.recs, 0xff, sizeof(SeamRec) * (size_t)pav_num_recs(n), s));   // s = -1: no hint from a previous iteration
    RBL_TRY(mem.alloc(&pw.counters, (size_t)PAV_COUNTERS));
    RBL_HIP(hipMemsetAsync(pw.counters, 0, PAV_COUNTERS * sizeof(u32), s));   // (read by every iteration's statistics, also when the caller supplied z)
    RBL_TRY(mem.alloc(&pw.partials, (size_t)reduce_blocks() * 4));
    RBL_TRY(mem.alloc(&pw.branch, 1));
    pw.ex = PavExtras{};
    RBL_TRY(mem.alloc(&pw.ex.bar, pav_bar_uints()));
    RBL_HIP(hipMemsetAsync(pw.ex.bar, 0, sizeof(unsigned) * pav_bar_uints(), s));
    // n bounds every launch on this workspace: the solver's z-step (n_total positions) and the distributed z-step, whose
    // chunk of the sorted order (zd_n) is at most n_total long (rbl_zd_prepare)
    RBL_TRY(mem.alloc(&pw.ex.big, (size_t)pav_big_recs(n)));
    RBL_TRY(mem.alloc(&pw.ex.fpart, (size_t)pav_fpart_doubles(n)));
    pw.ex.spec = 1;   // EHRM: branch b on every ADMM trajectory seen; corrected by the first exact test
    return RBL_OK;
}

int alloc_wstep(DevArena& mem, WstepWorkspace& ww, int64_t ld, hipStream_t s) {
    RBL_TRY(mem.alloc(&ww.yk, (size_t)ld));
    RBL_TRY(mem.alloc(&ww.Gy, (size_t)ld));
    RBL_TRY(mem.alloc(&ww.wn, (size_t)ld));
    RBL_TRY(mem.alloc(&ww.r, (size_t)ld));
    RBL_TRY(mem.alloc(&ww.p, (size_t)ld));
    RBL_TRY(mem.alloc(&ww.scal, 8));
    RBL_TRY(mem.alloc(&ww.flags, 8));
    RBL_TRY(mem.alloc(&ww.bar, (size_t)WSTEP_BAR_UINTS));
    RBL_HIP(hipMemsetAsync(ww.bar, 0, sizeof(unsigned) * WSTEP_BAR_UINTS, s));
    RBL_TRY(mem.alloc(&ww.xch, (size_t)WSTEP_XCH_DOUBLES));
    RBL_HIP(hipMemsetAsync(ww.xch, 0, sizeof(double) * WSTEP_XCH_DOUBLES, s));   // tag 0 is never used
    // the status blocks of the lasso kernel and of the CG batches live in pinned host memory the device
    // writes directly (status word last): the host spins on the word - no copy, no stream-wide wait
    RBL_TRY(mem.pinned(&ww.pin, 16, hipHostMallocCoherent));
    for (int i = 0; i < 16; ++i) ww.pin[i] = 0;
    return RBL_OK;
}

// own labels (rbl_set_labels): n host values between the handle's own sign convention and the owner's (an involution)
void flip_rows(const rbl_solver* h, double* x) {
    for (int64_t i = 0; i < h->n; ++i)
        if (h->rs_host[(size_t)i] < 0) x[i] = -x[i];
}

// n host doubles in the handle's own sign convention -> a device vector in the convention it is stored in (blocking)
int upload_rows(const rbl_solver* h, double* dst_dev, const double* src) {
    if (!h->rs) {
        RBL_HIP(hipMemcpy(dst_dev, src, sizeof(double) * h->n, hipMemcpyHostToDevice));
        return RBL_OK;
    }
    std::vector<double> t(src, src + h->n);
    flip_rows(h, t.data());
    RBL_HIP(hipMemcpy(dst_dev, t.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    return RBL_OK;
}

namespace {

double default_rho(int wf) {
    // src/optim/algorithms.py:47-52
    if (wf == RBL_W_EHRM) return 1e-4;
    if (wf == RBL_W_AORR || wf == RBL_W_AORR_DC) return 2e-7;
    return 1e-5;
}

int fill_const(double* p, int64_t count, double val, hipStream_t s) {
    std::vector<double> h((size_t)(count < (1 << 20) ? count : (1 << 20)), val);
    for (int64_t o = 0; o < count; o += (int64_t)h.size()) {
        int64_t c = count - o < (int64_t)h.size() ? count - o : (int64_t)h.size();
        RBL_HIP(hipMemcpyAsync(p + o, h.data(), sizeof(double) * c, hipMemcpyHostToDevice, s));
        RBL_HIP(hipStreamSynchronize(s));
    }
    return RBL_OK;
}

int validate(const rbl_config* c) {
    if (!c) {
        rbl_set_error("config is NULL");
        return RBL_ERR_INVALID;
    }
    if (c->n < 0 || c->d <= 0 || c->n_total < c->n || c->row_offset < 0 || c->row_offset + c->n > c->n_total) {
        rbl_set_error("bad shape: n=%lld d=%lld n_total=%lld row_offset=%lld", (long long)c->n, (long long)c->d,
                      (long long)c->n_total, (long long)c->row_offset);
        return RBL_ERR_INVALID;
    }
    if (c->n_total <= 0) {
        rbl_set_error("empty problem");
        return RBL_ERR_INVALID;
    }
    if (rbl_check_loss(c->loss) != RBL_OK) {   // (the text below replaces the check's own: it is the Python layer's)
        rbl_set_error("Unrecognized loss! Options: ['binary_cross_entropy', 'multinomial_cross_entropy', 'hinge', 'squared_hinge']");
        return RBL_ERR_INVALID;
    }
    if (c->weight_function < RBL_W_ERM || c->weight_function > RBL_W_EHRM) {
        rbl_set_error("Unrecognized framework! Options: ['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']");
        return RBL_ERR_INVALID;
    }
    if (c->has_B && c->loss != RBL_LOSS_BCE) {
        rbl_set_error("erhm only can be with the binary_cross_entropy.");  // objective.py:57-58
        return RBL_ERR_INVALID;
    }
    if (c->has_B && c->weight_function != RBL_W_EHRM) {
        rbl_set_error("Unrecognized weight_function! Options: ['ehrm']");  // algorithms.py:65-68
        return RBL_ERR_INVALID;
    }
    if (c->weight_function == RBL_W_EHRM && !c->objective_only && (!c->has_B || c->loss != RBL_LOSS_BCE)) {
        rbl_set_error("ehrm needs B and binary_cross_entropy");
        return RBL_ERR_INVALID;
    }
    if (c->weight_function != RBL_W_ERM && c->weight_function != RBL_W_EHRM) {
        const int need = (c->weight_function == RBL_W_AORR || c->weight_function == RBL_W_AORR_DC) ? 2 : 1;
        if (c->n_weight_args < need) {
            rbl_set_error("args for framework is None!");  // objective.py:171-172
            return RBL_ERR_INVALID;
        }
    }
    if (!c->objective_only) {
        if (c->wstep != RBL_WSTEP_L1 && c->wstep != RBL_WSTEP_L2 && c->wstep != RBL_WSTEP_SMOOTH_L1) {
            rbl_set_error("w_flag can only be 0, 1 or 2.");  // algorithms.py:206
            return RBL_ERR_INVALID;
        }
        if (!(c->reg > 0.0)) {
            rbl_set_error("l1_reg or l2_reg must be a positive number");
            return RBL_ERR_INVALID;
        }
    }
    if (c->storage != RBL_STORE_F32 && c->storage != RBL_STORE_F64 && c->storage != RBL_STORE_F16 && c->storage != RBL_STORE_CSR) {
        rbl_set_error("storage must be RBL_STORE_F32, RBL_STORE_F64, RBL_STORE_F16 or RBL_STORE_CSR");
        return RBL_ERR_INVALID;
    }
    if (c->storage == RBL_STORE_CSR && c->n != c->n_total) {
        rbl_set_error("RBL_STORE_CSR: row-sharded handles (n = %lld of n_total = %lld) are not supported - sparse storage runs "
                      "on one device", (long long)c->n, (long long)c->n_total);
        return RBL_ERR_INVALID;
    }
    if (c->storage == RBL_STORE_CSR && c->n > 0x7fffffffLL) {
        rbl_set_error("RBL_STORE_CSR: n = %lld exceeds 2^31 - 1 (row indices are 32 bits)", (long long)c->n);
        return RBL_ERR_INVALID;
    }
    if (c->n_total >= (1LL << 32)) {
        rbl_set_error("n_total must be < 2^32");
        return RBL_ERR_INVALID;
    }
    return RBL_OK;
}

// RBL_CREATE_NO_GRAM and what it asks of the problem; the late failure of a wide csr handle on the Gram route is refused here
int validate_gram_route(const rbl_config* c, uint32_t flags, const char* who) {
    const uint32_t known = RBL_CREATE_NO_GRAM | RBL_CREATE_WORKING_SET;
    if (flags & ~known) {
        rbl_set_error("%s: unknown flag bits 0x%x (RBL_CREATE_NO_GRAM = %d and RBL_CREATE_WORKING_SET = %d are the flags)", who,
                      flags & ~known, RBL_CREATE_NO_GRAM, RBL_CREATE_WORKING_SET);
        return RBL_ERR_INVALID;
    }
    if (flags & RBL_CREATE_WORKING_SET) {
        if (!(flags & RBL_CREATE_NO_GRAM)) {
            // (on a handle with a Gram matrix the bit means nothing: the message says so in the words of an unknown bit)
            rbl_set_error("%s: unknown flag bits 0x%x on a handle with a Gram matrix: RBL_CREATE_WORKING_SET needs "
                          "RBL_CREATE_NO_GRAM (the working set is the l1 w-step of a handle without a Gram matrix; the Gram "
                          "route has its exact active-set kernel already)", who, RBL_CREATE_WORKING_SET);
            return RBL_ERR_INVALID;
        }
        if (!c->objective_only && c->wstep != RBL_WSTEP_L1) {
            rbl_set_error("%s: RBL_CREATE_WORKING_SET needs cfg.wstep == RBL_WSTEP_L1 (the lasso / elastic-net w-step; got wstep %d)",
                          who, c->wstep);
            return RBL_ERR_INVALID;
        }
    }
    if (flags & RBL_CREATE_NO_GRAM) {
        if (c->storage != RBL_STORE_CSR) {
            rbl_set_error("%s: RBL_CREATE_NO_GRAM needs RBL_STORE_CSR (the operator w-step runs on the sparse passes; got storage %d)",
                          who, c->storage);
            return RBL_ERR_INVALID;
        }
        if (!c->objective_only && c->wstep == RBL_WSTEP_SMOOTH_L1) {
            rbl_set_error("%s: RBL_CREATE_NO_GRAM has no smoothed-l1 w-step (RBL_WSTEP_SMOOTH_L1 preconditions with diag(G), and "
                          "there is no Gram matrix on this route)", who);
            return RBL_ERR_INVALID;
        }
    } else if (c->storage == RBL_STORE_CSR && !c->objective_only && rbl_storage_ld(c->storage, c->d) > RBL_GRAM_MAX_LD) {
        rbl_set_error("%s: RBL_STORE_CSR with d = %lld: the Gram-space w-step holds a dense ld x ld matrix and stops at ld = %d - "
                      "create the handle with rbl_create_opts(cfg, RBL_CREATE_NO_GRAM, ...) (the operator w-step)", who,
                      (long long)c->d, RBL_GRAM_MAX_LD);
        return RBL_ERR_INVALID;
    }
    return RBL_OK;
}

int build_sigma_prefix(rbl_solver* h) {
    // sigma is static: its prefix sums are built once (pav.hip uses them every iteration)
    RBL_TRY(launch_prefix(h->sigma_a, h->nt, h->pfx_a, h->stream));
    if (h->cfg.weight_function == RBL_W_EHRM) RBL_TRY(launch_prefix(h->sigma_b, h->nt, h->pfx_b, h->stream));
    return RBL_OK;
}

}  // namespace

// ================================================================================ C ABI
extern "C" {

int rbl_version(void) { return RBL_VERSION; }

int rbl_wset_info(rbl_solver* h, rbl_wset_report* out) {
    RBL_ENTER_ITER(h);
    if (!out) {
        rbl_set_error("wset_info: out is NULL");
        return RBL_ERR_INVALID;
    }
    if (!h->wset) {
        rbl_set_error("wset_info: this handle has no working set (rbl_create_opts with RBL_CREATE_WORKING_SET)");
        return RBL_ERR_STATE;
    }
    *out = h->wset->rep;
    out->bytes = h->wset->bytes + (h->wset->Gs2 ? (int64_t)sizeof(double) * WS_CAP * WS_CAP : 0);
    return RBL_OK;
}

int rbl_sizeof(int which) {
    return which == 0 ? (int)sizeof(rbl_config) : which == 1 ? (int)sizeof(rbl_stats) : which == 2 ? (int)sizeof(rbl_wstep_report) :
           which == 3 ? (int)sizeof(rbl_gram_report) : -1;
}

const char* rbl_last_error(void) { return g_err.c_str(); }

int rbl_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cnt;
}

int rbl_destroy(rbl_solver* h) {
    if (!h) return RBL_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->kev) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->ev_spec) if (e) (void)hipEventDestroy(e);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->counted) g_live[h->cfg.device].fetch_sub(1, std::memory_order_relaxed);
    delete h;   // h->mem frees every buffer
    return RBL_OK;
}

}  // extern "C"

// everything rbl_create sets up past the checks of its arguments; on failure the caller destroys h
// owner != NULL: a borrower of owner's D and G (rbl_create_shared)
static int create_setup(rbl_solver* h, rbl_solver* owner = nullptr) {
    const rbl_config* cfg = &h->cfg;
    h->n = cfg->n;
    h->d = cfg->d;
    h->ld = rbl_storage_ld(cfg->storage, cfg->d);
    h->nt = cfg->n_total;
    h->off = cfg->row_offset;
    h->storage = cfg->storage;
    h->esz = rbl_storage_esz(cfg->storage);
    h->sorted_path = cfg->weight_function != RBL_W_ERM;
    // tol is taken literally, as the reference does (algorithms.py:137): tol <= 0 never reports convergence
    if (h->cfg.w_tol <= 0.0) h->cfg.w_tol = 1e-13;
    if (h->cfg.max_iter <= 0) h->cfg.max_iter = 200;
    hipDeviceProp_t prop;
    RBL_HIP(hipGetDeviceProperties(&prop, cfg->device));
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    RBL_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    for (auto& e : h->ev) RBL_HIP(hipEventCreate(&e));
    for (auto& e : h->kev) RBL_HIP(hipEventCreate(&e));
    for (auto& e : h->ev_spec) RBL_HIP(hipEventCreate(&e));
    DevArena& mem = h->mem;
    RBL_TRY(mem.pinned(&h->hstat, 16, hipHostMallocCoherent));
    h->fin.pin = reinterpret_cast<int*>(h->hstat + 15);
    const int64_t n = h->n, ld = h->ld, nt = h->nt;
    if (owner) {
        h->shared = owner->shared;
        h->gram_rep = owner->gram_rep;
        h->sd = owner->sd;
        h->borrower = true;
        h->D = owner->D;
        h->G = owner->G;
        h->ysign = owner->ysign;
        h->colstats = owner->colstats;
    } else {
        h->shared = std::make_shared<DevArena>();
        h->gram_rep = std::make_shared<rbl_gram_report>();
        h->sd = std::make_shared<SharedData>();
        const size_t dbytes = (size_t)(n > 0 ? n : 1) * ld * h->esz;
        if (h->storage == RBL_STORE_CSR) {
            // no n x ld matrix: D is the descriptor (stable - borrowers copy the pointer; read by the host alone, it only
            // shares the arena's life); the entry buffers it points at are allocated by rbl_set_data_csr, once nnz is known
            CsrStore* st = nullptr;
            RBL_TRY(h->shared->pinned(&st, 1, hipHostMallocDefault));
            memset(st, 0, sizeof(CsrStore));
            h->D = st;
        } else if (h->shared->alloc((unsigned char**)&h->D, dbytes) != RBL_OK) {
            rbl_set_error("hipMalloc of the %lld x %lld matrix (%zu bytes) failed: %s", (long long)n, (long long)ld, dbytes,
                          hipGetErrorString(hipGetLastError()));
            return RBL_ERR_NOMEM;
        }
        RBL_TRY(h->shared->alloc(&h->ysign, (size_t)n));
        RBL_TRY(h->shared->alloc(&h->colstats, (size_t)ld * 4));
        if (!cfg->objective_only && !h->no_gram) RBL_TRY(h->shared->alloc(&h->G, (size_t)ld * ld));
    }
    RBL_TRY(mem.alloc(&h->w, (size_t)ld));
    RBL_TRY(mem.alloc(&h->w_tmp, (size_t)ld));
    RBL_TRY(mem.alloc(&h->v, (size_t)n));
    RBL_TRY(mem.alloc(&h->m, (size_t)n));
    RBL_TRY(mem.alloc(&h->sigma_a, (size_t)nt));
    RBL_TRY(mem.alloc(&h->sigma_b, (size_t)nt));
    RBL_TRY(mem.alloc(&h->partials, (size_t)reduce_blocks() * 4));
    if (cfg->objective_only) RBL_TRY(mem.alloc(&h->red, 8));
    RBL_TRY(mem.alloc(&h->red2, 8));
    h->slab_bytes = (size_t)gemvt_slab_rows(h->num_cu) * ld * sizeof(double) * 2;
    // no Gram matrix: the slab only ever holds the segments' partial sums (ensure_sparse_slab grows it to the data), not
    // the dense passes' rows of ld - those are 800 MB at d = 200 000
    if (h->no_gram) h->slab_bytes = sizeof(double) * (size_t)ld;
    if (owner && h->storage == RBL_STORE_CSR)   // q = D^T c keeps one partial sum per segment in the handle's own slab
        h->slab_bytes = std::max(h->slab_bytes, sizeof(double) * (size_t)((const CsrStore*)owner->D)->nseg);
    if (!cfg->objective_only) {
        size_t gb = owner || h->no_gram ? 0 : gram_slab_bytes(ld, h->num_cu, n > 0 ? n : 1);   // (a borrower never forms G)
        if (gb > h->slab_bytes) h->slab_bytes = gb;
        RBL_TRY(mem.alloc(&h->w_prev, (size_t)ld));
        // one exchange buffer, summed over ranks in at most one collective per iteration:
        // [q (ld) | D^T lambda seed (ld) | ||z||^2 | primal^2 | sum loss]
        RBL_TRY(mem.alloc(&h->q, (size_t)ld * 2 + 3));
        h->red = h->q + 2 * ld + 1;
        RBL_TRY(mem.alloc(&h->z, (size_t)n));
        RBL_TRY(mem.alloc(&h->lam, (size_t)n));
        RBL_TRY(mem.alloc(&h->c, (size_t)n));
        RBL_TRY(alloc_wstep(mem, h->ww, ld, h->stream));
        if (h->no_gram) {   // the operator's n-vector and the chunk partials of its d-space kernels
            RBL_TRY(mem.alloc(&h->op_t, (size_t)(n > 0 ? n : 1)));
            RBL_TRY(mem.alloc(&h->op_part, op_part_doubles(ld)));
            if (h->working_set) {
                h->wset.reset(new WsetState());
                RBL_TRY(alloc_wset(mem, *h->wset, ld, h->stream));
            }
        }
    }
    RBL_TRY(mem.alloc((unsigned char**)&h->slab, h->slab_bytes));
    if (h->sorted_path) {
        RBL_TRY(alloc_sort(mem, h->sw, nt, !cfg->objective_only, h->stream));
        if (!cfg->objective_only) {
            RBL_TRY(alloc_pav(mem, h->pw, nt, h->stream));
            RBL_TRY(mem.alloc(&h->s32.mm, (size_t)s32_range_words()));
            RBL_TRY(mem.alloc(&h->s32.flag, 1));
            RBL_TRY(mem.pinned(&h->s32.v.pin, 16, hipHostMallocDefault));
            for (int i = 0; i < 16; ++i) h->s32.v.pin[i] = 0;
            RBL_TRY(alloc_prefix(mem, h->pfx_a, nt));
            h->pfx_b = h->pfx_a;
            if (cfg->weight_function == RBL_W_EHRM) RBL_TRY(alloc_prefix(mem, h->pfx_b, nt));
        }
    }
    // sigma (objective.py:46-54): alphas, betas (= alphas unless ehrm)
    RBL_TRY(launch_weights(cfg->weight_function, nt, cfg->weight_args, h->sigma_a, h->sigma_b, h->stream));
    h->sigma0 = 1.0 / (double)nt;
    if (h->sorted_path && !cfg->objective_only) RBL_TRY(build_sigma_prefix(h));
    // initial state, algorithms.py:32-52 (n = num_row of the WHOLE problem)
    RBL_HIP(hipMemsetAsync(h->w, 0, sizeof(double) * ld, h->stream));
    RBL_HIP(hipMemsetAsync(h->w_tmp, 0, sizeof(double) * ld, h->stream));
    if (!cfg->objective_only) {
        const double reg = cfg->reg;
        RBL_TRY(fill_const(h->lam, n, 0.1 * reg / (double)nt, h->stream));
        RBL_TRY(fill_const(h->z, n, 0.1 * reg / (double)nt, h->stream));
        RBL_TRY(fill_const(h->w, h->d, 0.001 * reg / (double)h->d / (double)nt, h->stream));
        RBL_HIP(hipMemsetAsync(h->q, 0, sizeof(double) * (ld * 2 + 3), h->stream));
        h->fused_ok = single_sweep_allowed(h);
        h->fuse_v = !h->fused_ok && !no_fuse() && n > 0 && sweep_v_supported(h->storage, ld);
        if (h->fused_ok) {
            RBL_TRY(mem.alloc(&h->z_next, (size_t)n));
            RBL_TRY(mem.alloc(&h->p, (size_t)ld));
            RBL_TRY(mem.alloc(&h->p_alt, (size_t)ld));
            RBL_TRY(mem.alloc(&h->pred, 2));
        }
        h->rho = cfg->rho0 > 0.0 ? cfg->rho0 : default_rho(cfg->weight_function);
        h->smooth_t = cfg->smooth_t > 0.0 ? cfg->smooth_t : 1.0;
    }
    if (owner) {
        h->data_ready = true;
        RBL_TRY(sync_data_epoch(h));   // a new handle is behind every epoch: it takes what the owner derived from G alone
    } else {
        h->epoch = h->sd->epoch;
    }
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

extern "C" {

int rbl_create_shared(const rbl_config* cfg, rbl_solver* owner, rbl_solver** out) {
    if (!out) {
        rbl_set_error("out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = nullptr;
    RBL_TRY(validate(cfg));
    if (!owner) {
        rbl_set_error("create_shared: owner is NULL");
        return RBL_ERR_INVALID;
    }
    const rbl_config& oc = owner->cfg;
    if (cfg->n != oc.n || cfg->d != oc.d || cfg->n_total != oc.n_total || cfg->row_offset != oc.row_offset ||
        cfg->storage != oc.storage || cfg->device != oc.device) {
        rbl_set_error("create_shared: config disagrees with the owner (n=%lld/%lld d=%lld/%lld n_total=%lld/%lld row_offset=%lld/%lld "
                      "storage=%d/%d device=%d/%d)", (long long)cfg->n, (long long)oc.n, (long long)cfg->d, (long long)oc.d,
                      (long long)cfg->n_total, (long long)oc.n_total, (long long)cfg->row_offset, (long long)oc.row_offset,
                      cfg->storage, oc.storage, cfg->device, oc.device);
        return RBL_ERR_INVALID;
    }
    // a borrower of a no-Gram owner is a no-Gram handle: its cfg follows the rules of the flag
    RBL_TRY(validate_gram_route(cfg, (owner->no_gram ? RBL_CREATE_NO_GRAM : 0) | (owner->working_set ? RBL_CREATE_WORKING_SET : 0),
                                "create_shared"));
    if (!owner->data_ready) {
        rbl_set_error("create_shared: the owner has no data yet (rbl_set_data / rbl_generate_synthetic first)");
        return RBL_ERR_STATE;
    }
    if (!cfg->objective_only && !owner->no_gram && (!owner->der.gram_ready || !owner->G)) {
        rbl_set_error("create_shared: the owner's Gram matrix is not ready (rbl_gram_local + rbl_gram_finish first)");
        return RBL_ERR_STATE;
    }
    if (!cfg->objective_only && owner->no_gram && (owner->cfg.objective_only || !owner->der.gram_ready)) {
        rbl_set_error("create_shared: the owner's step constant is not ready (rbl_gram_local + rbl_gram_finish first; an "
                      "objective-only owner has none)");
        return RBL_ERR_STATE;
    }
    RBL_TRY(check_device(nullptr));
    RBL_HIP(hipSetDevice(oc.device));
    RBL_HIP(hipStreamSynchronize(owner->stream));   // D and G are complete before another stream reads them
    rbl_solver* h = new rbl_solver();
    h->cfg = *cfg;
    h->no_gram = owner->no_gram;
    h->working_set = owner->working_set;
    if (cfg->device < 64) {
        g_live[cfg->device].fetch_add(1, std::memory_order_relaxed);
        h->counted = true;
    }
    const int rc = create_setup(h, owner);
    if (rc != RBL_OK) {
        rbl_destroy(h);
        return rc;
    }
    *out = h;
    return RBL_OK;
}

int rbl_create_opts(const rbl_config* cfg, uint32_t flags, rbl_solver** out) {
    if (!out) {
        rbl_set_error("out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = nullptr;
    RBL_TRY(validate(cfg));
    RBL_TRY(validate_gram_route(cfg, flags, flags ? "create_opts" : "create"));
    int cnt = 0;
    RBL_TRY(check_device(&cnt));
    if (cfg->device < 0 || cfg->device >= cnt) {
        rbl_set_error("device %d out of range (%d devices)", cfg->device, cnt);
        return RBL_ERR_INVALID;
    }
    RBL_HIP(hipSetDevice(cfg->device));
    rbl_solver* h = new rbl_solver();
    h->cfg = *cfg;
    h->no_gram = (flags & RBL_CREATE_NO_GRAM) != 0;
    h->working_set = (flags & RBL_CREATE_WORKING_SET) != 0;
    if (cfg->device < 64) {
        g_live[cfg->device].fetch_add(1, std::memory_order_relaxed);
        h->counted = true;
    }
    const int rc = create_setup(h);
    if (rc != RBL_OK) {
        rbl_destroy(h);
        return rc;
    }
    *out = h;
    return RBL_OK;
}

int rbl_create(const rbl_config* cfg, rbl_solver** out) { return rbl_create_opts(cfg, 0, out); }

int rbl_set_stream(rbl_solver* h, void* hip_stream) {
    RBL_ENTER(h);
    RBL_HIP(hipStreamSynchronize(h->stream));
    // NULL is a real stream (the legacy default stream torch uses unless told otherwise);
    // (void*)-1 restores the handle's own non-blocking stream
    h->stream = (hip_stream == (void*)-1) ? h->own_stream : (hipStream_t)hip_stream;
    return RBL_OK;
}

int rbl_get_state(rbl_solver* h, double* w, double* z, double* lam, double* rho, int64_t* iter, double* smooth_t) {
    RBL_ENTER_ITER(h);
    // a reader of z between rbl_phase_z and rbl_phase_w (an overridden w_subproblem) gets a certified z: a verdict of the
    // sort-free z-step or of the 32-bit sort that is still pending is settled here, the step redone if it says so
    if (z && h->z) RBL_TRY(zb_resolve(h));
    RBL_HIP(hipStreamSynchronize(h->stream));
    // while the next w-step is in flight ahead of time, the current iterate w_k is w_prev
    if (w) RBL_HIP(hipMemcpy(w, h->spec_w ? h->w_prev : h->w, sizeof(double) * h->d, hipMemcpyDeviceToHost));
    if (z && h->z) RBL_HIP(hipMemcpy(z, h->z, sizeof(double) * h->n, hipMemcpyDeviceToHost));
    if (lam && h->lam) RBL_HIP(hipMemcpy(lam, h->lam, sizeof(double) * h->n, hipMemcpyDeviceToHost));
    if (h->rs) {   // the caller sees the handle's own sign convention
        if (z && h->z) flip_rows(h, z);
        if (lam && h->lam) flip_rows(h, lam);
    }
    if (rho) *rho = h->rho;
    if (iter) *iter = h->iter;
    if (smooth_t) *smooth_t = h->smooth_t;
    return RBL_OK;
}

int rbl_set_state(rbl_solver* h, const double* w, const double* z, const double* lam, const double* rho,
                  const int64_t* iter, const double* smooth_t) {
    RBL_ENTER(h);
    RBL_HIP(hipStreamSynchronize(h->stream));
    if (w) {
        RBL_HIP(hipMemcpy(h->w, w, sizeof(double) * h->d, hipMemcpyHostToDevice));
        w_changed(h->der);
        if (h->wset) h->wset->w_replaced();   // any S that holds the new support is valid: the next w-step finds it
    }
    if (z && h->z) {
        RBL_TRY(upload_rows(h, h->z, z));
        z_replaced(h->der);
    }
    if (lam && h->lam) {
        RBL_TRY(upload_rows(h, h->lam, lam));
        lambda_changed(h->der);
    }
    if (rho) {
        h->rho = *rho;
        rho_changed(h->der);
    }
    if (iter) h->iter = *iter;
    if (smooth_t) h->smooth_t = *smooth_t;
    return RBL_OK;
}

int rbl_get_sigma(rbl_solver* h, double* alphas, double* betas) {
    RBL_ENTER(h);
    RBL_HIP(hipStreamSynchronize(h->stream));
    if (alphas) RBL_HIP(hipMemcpy(alphas, h->sigma_a, sizeof(double) * h->nt, hipMemcpyDeviceToHost));
    if (betas) RBL_HIP(hipMemcpy(betas, h->sigma_b, sizeof(double) * h->nt, hipMemcpyDeviceToHost));
    return RBL_OK;
}

int rbl_buffer(rbl_solver* h, int which, void** dev_ptr, int64_t* n_doubles) {
    RBL_ENTER(h);
    void* p = nullptr;
    int64_t cnt = 0;
    switch (which) {
        case RBL_BUF_M: p = h->m; cnt = h->n; break;
        case RBL_BUF_Q: p = h->q; cnt = h->q ? 2 * h->ld + 3 : 0; break;  // whole exchange buffer (RED = its tail)
        case RBL_BUF_RED: p = h->red; cnt = 2; break;
        case RBL_BUF_G:
            if (h->no_gram) {
                rbl_set_error("buffer(RBL_BUF_G): this handle has no Gram matrix (RBL_CREATE_NO_GRAM: the operator w-step)");
                return RBL_ERR_STATE;
            }
            p = h->G;
            cnt = h->ld * h->ld;
            break;
        case RBL_BUF_V: p = h->v; cnt = h->n; break;
        case RBL_BUF_Z: p = h->z; cnt = h->n; break;
        case RBL_BUF_LAM: p = h->lam; cnt = h->n; break;
        case RBL_BUF_W: p = h->w; cnt = h->ld; break;
        case 8: p = h->colstats; cnt = 2 * h->ld; break;  // RBL_BUF_COLSTATS
        // distributed z-step: typed views (element counts; int64 / int32 / double as rbl.h says)
        case RBL_BUF_ZD_SKEYS: p = h->sorted_path ? h->sw.keys[0] : nullptr; cnt = h->n; break;
        case RBL_BUF_ZD_SIDS: p = h->sorted_path ? h->sw.vals[0] : nullptr; cnt = h->n; break;
        case RBL_BUF_ZD_RKEYS: p = h->sorted_path ? h->sw.keys[1] : nullptr; cnt = h->nt; break;
        case RBL_BUF_ZD_RIDS: p = h->sorted_path ? h->sw.vals[1] : nullptr; cnt = h->nt; break;
        case RBL_BUF_ZD_SMALL: RBL_TRY(zd_ensure(h)); p = h->zd_small; cnt = ZD_SMALL_DOUBLES; break;
        case RBL_BUF_ZD_BIDS: p = h->sorted_path ? h->sw.vals[1] : nullptr; cnt = h->nt; break;
        case RBL_BUF_ZD_BU: p = h->sorted_path ? h->sw.keys[1] : nullptr; cnt = h->nt; break;
        case RBL_BUF_ZD_ZIDS: RBL_TRY(zd_ensure(h)); p = h->zd_zids; cnt = h->n; break;
        case RBL_BUF_ZD_ZU: p = h->m; cnt = h->n; break;
        case RBL_BUF_ZD_COUNTS: RBL_TRY(zd_ensure(h)); p = h->zd_counts_dev; cnt = 64; break;
        case RBL_BUF_ZB_HIST: p = h->zb.hist; cnt = h->zb.hist ? (int64_t)(zb_hist_bytes() / sizeof(u32)) : 0; break;
        case RBL_BUF_ZB_TOT: p = h->zb.tot; cnt = h->zb.tot ? 4 * ZB_C : 0; break;
        case RBL_BUF_ZB_PACK: p = h->zb.pack; cnt = h->zb.pack ? ZB_GCAP + 1 : 0; break;
        default: rbl_set_error("unknown buffer id %d", which); return RBL_ERR_INVALID;
    }
    if (dev_ptr) *dev_ptr = p;
    if (n_doubles) *n_doubles = cnt;
    return RBL_OK;
}

int rbl_kernel_time(rbl_solver* h, int which, double* total_ms, int64_t* launches) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (which == RBL_KERNEL_SRC_STATS || which == RBL_KERNEL_SRC_FORM) {   // the last rbl_set_data_from
        if (total_ms) *total_ms = h->src_ms[which - RBL_KERNEL_SRC_STATS];
        if (launches) *launches = h->src_timed[which - RBL_KERNEL_SRC_STATS];
        return RBL_OK;
    }
    if (which < 0 || which > 2) return RBL_ERR_INVALID;
    if (total_ms) *total_ms = h->kt_ms[which];
    if (launches) *launches = h->kt_n[which];
    return RBL_OK;
}

int rbl_reset_kernel_times(rbl_solver* h) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    h->kt_ms[0] = h->kt_ms[1] = h->kt_ms[2] = 0.0;
    h->kt_n[0] = h->kt_n[1] = h->kt_n[2] = 0;
    for (auto& v : h->kt_samples) v.clear();
    return RBL_OK;
}

int rbl_kernel_samples(rbl_solver* h, int which, double* out_ms, int64_t cap, int64_t* count) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (which < 0 || which > 2 || cap < 0 || (cap > 0 && !out_ms)) return RBL_ERR_INVALID;
    const std::vector<float>& v = h->kt_samples[which];
    const int64_t k = (int64_t)v.size() < cap ? (int64_t)v.size() : cap;
    for (int64_t i = 0; i < k; ++i) out_ms[i] = (double)v[(size_t)i];
    if (count) *count = (int64_t)v.size();
    return RBL_OK;
}

int rbl_profile_kernels(rbl_solver* h, int enable) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    h->profile = enable != 0;
    h->phase_timing = enable >= 2;
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

int rbl_profile_sampling(rbl_solver* h, int every) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (every < 1) {
        rbl_set_error("profile_sampling: every must be >= 1");
        return RBL_ERR_INVALID;
    }
    h->profile_every = every;
    return RBL_OK;
}

// which part of the exchange buffer (RBL_BUF_Q) has to be summed over the ranks right now:
// bit 0 = q part [0, 2 ld + 1), bit 1 = residual part [2 ld + 1, 2 ld + 3)
int rbl_pending_reduce(rbl_solver* h, int* mask) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (mask) *mask = h->pending_mask;
    return RBL_OK;
}

int rbl_info(rbl_solver* h, int64_t* ld, int* num_cu, double* lipschitz) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (ld) *ld = h->ld;
    if (num_cu) *num_cu = h->num_cu;
    if (lipschitz) *lipschitz = h->L;
    return RBL_OK;
}

}  // extern "C"
