// api.hip - the C ABI of librbl.so (include/rbl.h): solver handle, data path, the ADMM
// iteration of src/optim/algorithms.py:119-164 as a sequence of device phases, and the
// kernel-level entry points used by the parity tests.  Host code only orchestrates:
// every arithmetic step runs in a HIP kernel; there is no CPU fallback.
#include "rbl_internal.h"

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <utility>
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

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

struct rbl_solver {
    DevArena mem;   // every device and pinned buffer of the handle's own (per-problem) state
    // what depends on (X, y) alone - D, G, the labels, the column statistics, the eigenbasis of G - lives in an arena of
    // its own: the handle that uploaded the data and the handles that borrow it (rbl_create_shared) hold it together,
    // the last one to go frees it
    std::shared_ptr<DevArena> shared;
    bool borrower = false;         // D and G are another handle's: no upload, no Gram launch on this one
    int64_t nd_launches = 0;       // n x d launches this handle ran for itself (rbl_group_counters: single_passes)
    bool in_group = false;         // member of an rbl_group: runs on the group's stream, erm without the single-sweep pass
    rbl_config cfg;
    bool counted = false;
    int64_t n = 0, d = 0, ld = 0, nt = 0, off = 0;
    int storage = 0;
    size_t esz = 4;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    int num_cu = 256;
    bool data_ready = false, gram_ready = false, gram_local_done = false, v_valid = false;
    bool sorted_path = false;  // weight function needs sort + PAV

    void* D = nullptr;
    double *w = nullptr, *w_prev = nullptr, *q = nullptr, *G = nullptr, *w_tmp = nullptr;
    double *z = nullptr, *lam = nullptr, *v = nullptr, *m = nullptr, *c = nullptr;
    double *sigma_a = nullptr, *sigma_b = nullptr;
    double *slab = nullptr;
    size_t slab_bytes = 0;
    double *partials = nullptr, *red = nullptr, *red2 = nullptr;
    signed char* ysign = nullptr;
    // labels of this handle's own on a borrowed D (rbl_set_labels): rs[i] = y_i * y_owner_i, one byte per row in this
    // handle's arena; NULL = the owner's labels.  v, z, lambda, c are then kept in the OWNER's sign convention (z~ = r z,
    // lambda~ = r lambda, c~ = r c; v = D w as the passes over the owner's D leave it), m is the true m; the sign is taken
    // out by the element-wise kernels around the z-step and the losses.  rs_host / ys_host: r and the own labels on the host
    signed char* rs = nullptr;
    std::vector<signed char> rs_host, ys_host;
    double* colstats = nullptr;  // [sum(ld) | sumsq(ld) | mean(ld) | inv_std(ld)]

    SortWorkspace sw{};
    PavWorkspace pw{};
    PrefixBufs pfx_a, pfx_b;   // prefix sums of sigma_a / sigma_b (pfx_b = pfx_a unless EHRM)
    WstepWorkspace ww{};
    double L = 0.0;

    // host-side state of the iteration (algorithms.py:32-52)
    double rho = 0.0, smooth_t = 1.0, sigma0 = 0.0;
    int64_t iter = 0;
    // scratch of the step in flight
    double step_rho = 0.0;
    int inner_iters = 0;
    int want_obj = 0;
    bool obj_is_risk = false;

    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t kev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // gemv, gemvt, sweep_erm: begin/end
    bool profile = false, kev_pending[3] = {false, false, false};
    int profile_every = 1;   // kernel events on every profile_every-th iteration (rbl_profile_sampling)
    double kt_ms[3] = {0.0, 0.0, 0.0};
    int64_t kt_n[3] = {0, 0, 0};
    std::vector<float> kt_samples[3];   // the timed launches one by one, in order (rbl_kernel_samples)

    // single-sweep erm iteration (sweep_erm.hip)
    bool fused_ok = false, z_ready = false, p_valid = false, p_pending = false, pred_valid = false, fused_ran = false;
    // distributed z-step (rbl_zd_*): this rank's chunk of the globally sorted order
    double* zd_small = nullptr;      // samples | bounds | fvals | candidates | partial sums | seam sums
    ZdSeam* zd_seam = nullptr;
    int* zd_err = nullptr;
    long long* zd_bounds_dev = nullptr;
    long long* zd_counts_dev = nullptr;   // RBL_BUF_ZD_COUNTS: per-destination counts of the sample sort (64 x int64)
    u32* zd_zids = nullptr;          // row ids received back (n)
    PrefixBufs zd_a, zd_b;           // prefix sums of the chunk's slice of sigma_a / sigma_b (zd_b = zd_a unless EHRM)
    int64_t zd_n = 0, zd_off = 0;    // chunk length and its offset in the sorted order
    int zd_world = 0;
    bool fuse_v = false;   // rank-weighted problems: v = D w fused with the lambda update (sweep_erm.hip, SE_VONLY)
    int pending_mask = 0;  // bit 0: the q part, bit 1: the residual part of the exchange buffer awaits a sum over ranks
    double *z_next = nullptr, *p = nullptr, *p_alt = nullptr, *pred = nullptr;
    double* hstat = nullptr;   // pinned host block the end-of-iteration statistics are packed into by the device
    // The lasso w-step of iteration k+1 is enqueued by rbl_phase_finish(k) before the host has
    // read iteration k's statistics (its inputs q and rho_{k+1} = pred[0] are already on the
    // device); spec_w says that w currently holds that speculative w_{k+1} (w_prev = w_k).
    bool spec_w = false, spec_timed = false;
    hipEvent_t ev_spec[2] = {nullptr, nullptr};
    bool phase_timing = false;   // rbl_profile_kernels level 2: HIP events around the phases (ms_* of rbl_stats)
    int64_t n_fused = 0, n_mispred = 0;
    bool fused_v_ran = false;
    int eig_sweeps = 0;    // Jacobi sweeps of the one-time eigendecomposition of G (l2 w-step), 0 = CG is used
    bool keys_ready = false;   // rbl_phase_m left the sort's input (keys of m, global row ids) in sw.keys[0] / vals[0]
    // z-step with 32-bit sort keys (round 3; elementwise.hip: k_keys32 / k_sort32_fix): rbl_phase_m left m and its range
    // (m32_ready); the sort's verdict - no run of equal keys too long to repair - arrives in pinned memory like the
    // sort-free z-step's and is settled by the same entries (zb_resolve): not certified = redone with 64-bit keys
    struct {
        bool m_ready = false, used = false, q_done = false;
        u64* mm = nullptr;       // range of m (device)
        int* flag = nullptr;     // device: 1 = a run too long
        int* pin = nullptr;      // pinned: [0] sequence number (written last), [1] flag
        int seq = 0;
        int64_t skip_until = 0;
    } s32;
    int sort_passes = 0;   // radix passes executed by the z-step in flight
    // z-step without a sort for piecewise-constant rank weights (zband.hip); `used`: this iteration's z came from it
    // and its status word has not been looked at yet
    struct {
        bool checked = false, enabled = false, used = false, c_ready = false, q_done = false;
        ZbConfig cfg;
        ZbState* st = nullptr;
        u32* hist = nullptr;
        double* part = nullptr;
        double* tot = nullptr;     // multi-GPU: the sums of one root pass (all-reduced by the driver)
        double* pack = nullptr;    // multi-GPU: [count | undecided elements] of this rank (all-gathered by the driver)
        int* pin = nullptr;    // pinned: [0] sequence number (written last), [1] status
        int seq = 0, mode = 0, dseq = 0;
        int64_t backoff = 0, skip_until = 0;   // after an uncertified z-step the fast path pauses for 2, 4, ... 64 iterations   // mode of the iteration in flight: 0 sort, 1 banded, 2 banded then redone with the sort
    } zb;
};

static thread_local int g_host_syncs = 0;   // one solver handle per host thread (include/rbl.h)
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

namespace {

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

double default_rho(int wf) {
    // src/optim/algorithms.py:47-52
    if (wf == RBL_W_EHRM) return 1e-4;
    if (wf == RBL_W_AORR || wf == RBL_W_AORR_DC) return 2e-7;
    return 1e-5;
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

int fill_const(double* p, int64_t count, double val, hipStream_t s) {
    std::vector<double> h((size_t)(count < (1 << 20) ? count : (1 << 20)), val);
    for (int64_t o = 0; o < count; o += (int64_t)h.size()) {
        int64_t c = count - o < (int64_t)h.size() ? count - o : (int64_t)h.size();
        RBL_HIP(hipMemcpyAsync(p + o, h.data(), sizeof(double) * c, hipMemcpyHostToDevice, s));
        RBL_HIP(hipStreamSynchronize(s));
    }
    return RBL_OK;
}

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
    if (c->loss != RBL_LOSS_BCE && c->loss != RBL_LOSS_HINGE) {
        rbl_set_error("Unrecognized loss! Options: ['binary_cross_entropy', 'multinomial_cross_entropy', 'hinge']");
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
    if (c->storage != RBL_STORE_F32 && c->storage != RBL_STORE_F64) {
        rbl_set_error("storage must be RBL_STORE_F32 or RBL_STORE_F64");
        return RBL_ERR_INVALID;
    }
    if (c->n_total >= (1LL << 32)) {
        rbl_set_error("n_total must be < 2^32");
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

int ensure_v(rbl_solver* h) {
    if (h->v_valid) return RBL_OK;
    h->nd_launches += 1;
    RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w, h->v, h->num_cu, h->stream));
    h->v_valid = true;
    return RBL_OK;
}

// written by one thread behind the 32-bit sort's fix-up: its verdict for the host (sequence number last)
static __global__ void k_publish_flag(const int* __restrict__ flag, int* __restrict__ pin, int seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    pin[1] = flag[0];
    __threadfence_system();
    reinterpret_cast<volatile int*>(pin)[0] = seq;
}

// Sorted-path z-step over the n_total values in msrc (device), writing the local slice.
// allow32: the 32-bit-key sort may be used when rbl_phase_m prepared it (h->s32.m_ready) - its verdict is settled later
// (zb_resolve); false: 64-bit keys (the redo of an uncertified step, gathered m of the replicated distributed form).
int z_step_sorted(rbl_solver* h, const double* msrc, double rho, bool allow32 = true) {
    hipStream_t s = h->stream;
    const int64_t nt = h->nt;
    const u32* perm = h->sw.vals[0];
    const bool use32 = allow32 && h->s32.m_ready && msrc == h->m && nt == h->n;
    h->s32.m_ready = false;
    if (use32) {
        // fixed-point 32-bit keys of m: 4 radix passes over 8 bytes per row instead of 8 over 12, then one pass that gathers
        // the sorted m through the row ids and repairs the short runs the 32 bits cannot tell apart
        u32* k32 = reinterpret_cast<u32*>(h->sw.keys[0]);
        RBL_TRY(launch_keys32(nt, h->m, h->s32.mm, k32, h->sw.vals[0], (u32)h->off, s));
        RBL_TRY(launch_radix_sort32(h->sw, nt, s));
        RBL_TRY(launch_sort32_fix(nt, k32, h->sw.vals[0], h->m, (u32)h->off, h->pw.ms, h->sw.vals[1], h->s32.flag, s));
        h->s32.seq = (h->s32.seq & 0x3fffffff) + 1;
        h->s32.pin[0] = 0;
        hipLaunchKernelGGL(k_publish_flag, dim3(1), dim3(64), 0, s, (const int*)h->s32.flag, h->s32.pin, h->s32.seq);
        RBL_HIP(hipGetLastError());
        h->s32.used = true;
        h->s32.q_done = false;
        RBL_TRY(launch_prefix(h->pw.ms, nt, h->pw.pm, s));
        perm = h->sw.vals[1];
        h->sort_passes += 4;
    } else {
        // rbl_phase_m already formed the keys with m when it covers the whole problem (one pass instead of two)
        if (!(h->keys_ready && msrc == h->m && nt == h->n)) RBL_TRY(launch_keys_from_m(nt, msrc, h->sw.keys[0], h->sw.vals[0], s));
        RBL_TRY(launch_radix_sort(h->sw, nt, true, s));
        RBL_TRY(launch_unflip_prefix(h->sw.keys[0], nt, h->pw.ms, h->pw.pm, s));
        h->sort_passes += 8;
    }
    h->keys_ready = false;   // the sort consumes its input
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    // EHRM: the branch of the previous iteration is speculated and the exact test rides on the bottom kernel
    // (pav.hip: k_pav_bottom<0, true>).  RBL_EHRM_SPEC=0 / 1: the first speculation (tests force a wrong one);
    // RBL_EHRM_SPEC=-1: round 2's form - a pass of its own solves both element prox problems (k_ehrm_fvals), the tree
    // reads the chosen one as its level 0
    int spec_env = 2;
    if (ehrm) {
        const char* e = getenv("RBL_EHRM_SPEC");   // (read per z-step: the tests switch it between handles)
        if (e) spec_env = atoi(e);
    }
    PavExtras ex = h->pw.ex;
    ex.num_cu = h->num_cu;
    ex.B = h->cfg.B;
    const bool spec = ehrm && spec_env != -1;
    if (!spec) ex.fpart = nullptr;
    if (spec && h->iter == 0 && (spec_env == 0 || spec_env == 1)) ex.spec = spec_env;
    double* u0a = (ehrm && !spec) ? h->pw.u : nullptr;
    double* u0b = (ehrm && !spec) ? (double*)h->sw.keys[1] : nullptr;   // free once the sort is done
    if (ehrm && !spec)
        RBL_TRY(launch_ehrm_branch(nt, h->sigma_a, h->sigma_b, h->cfg.B, rho, h->pw.ms, h->pw.partials, h->pw.branch,
                                   -1, s, u0a, u0b));
    RBL_TRY(launch_pav_tree(h->cfg.loss, nt, rho, h->pw.ms, h->sigma_a, h->sigma_b, h->pw.u, h->pfx_a.view(), h->pfx_b.view(),
                            h->pw.pm.view(), ehrm ? h->pw.branch : nullptr, h->pw.recs, h->pw.counters, s, u0a, u0b, &ex));
    h->pw.ex.bar_parity = ex.bar_parity;
    RBL_TRY(launch_scatter_z(nt, h->pw.u, perm, ehrm ? h->pw.branch : nullptr, h->cfg.B, ehrm ? 1 : 0, rho,
                             h->lam, h->z, nullptr, h->off, h->n, s, h->rs));
    return RBL_OK;
}

// Are the rank weights constant on a few bands (superquantile, aorr, aorr_dc)?  Then the z-step needs no sort
// (zband.hip).  Looked at once per handle, at the first rank-weighted z-step.
int zb_setup(rbl_solver* h) {
    h->zb.checked = true;
    h->zb.enabled = false;
    const char* off = getenv("RBL_NO_ZBAND");
    if (off && off[0] == '1') return RBL_OK;
    const char* mn = getenv("RBL_ZBAND_MIN_N");
    const long long min_n = mn ? atoll(mn) : 4096;   // (6000 x 1000: 0.47 against 0.63 ms per iteration; below a few thousand rows nothing is gained)
    // (the configuration speaks of GLOBAL ranks: a row-sharded handle builds the same one; its driver runs the steps with
    // collectives in between - rbl_zbd_*)
    if (!h->sorted_path || h->cfg.weight_function == RBL_W_EHRM || h->nt < min_n || h->nt < 16) return RBL_OK;
    constexpr int CAP = 16;
    long long pos[CAP];
    int cnt = 0;
    {
        DevArena tmp;   // the edge buffers, freed once read back
        long long* pos_dev = nullptr;
        int* cnt_dev = nullptr;
        RBL_TRY(tmp.alloc(&pos_dev, (size_t)CAP));
        RBL_TRY(tmp.alloc(&cnt_dev, (size_t)1));
        int rc = launch_zb_edges(h->sigma_a, h->nt, pos_dev, cnt_dev, CAP, h->stream);
        if (rc == RBL_OK && (hipMemcpyAsync(&cnt, cnt_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                             hipMemcpyAsync(pos, pos_dev, sizeof(pos), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                             hipStreamSynchronize(h->stream) != hipSuccess))
            rc = RBL_ERR_HIP;
        if (rc != RBL_OK) {
            rbl_set_error("zband setup: reading the edges of sigma failed");
            return rc;
        }
    }
    if (cnt < 1 || cnt > ZB_MAX_BANDS - 1) return RBL_OK;   // constant weights never come here (erm); smooth families: sort
    std::sort(pos, pos + cnt);
    ZbConfig& c = h->zb.cfg;
    std::memset(&c, 0, sizeof(c));
    c.nbands = cnt + 1;
    c.start[0] = 0;
    for (int j = 0; j < cnt; ++j) c.start[j + 1] = pos[j];
    c.start[c.nbands] = h->nt;
    for (int j = 0; j < c.nbands; ++j)
        RBL_HIP(hipMemcpy(&c.sigma[j], h->sigma_a + c.start[j], sizeof(double), hipMemcpyDeviceToHost));
    auto size = [&](int j) { return c.start[j + 1] - c.start[j]; };
    if (size(0) < 2 || size(c.nbands - 1) < 2) return RBL_OK;
    // targets: last rank of every band but the last, first rank of every band but the first (ascending, unique)
    auto add_target = [&](long long r) {
        for (int t = 0; t < c.ntargets; ++t)
            if (c.target_rank[t] == r) return t;
        if (c.ntargets == ZB_MAX_TARGETS) return -1;
        c.target_rank[c.ntargets] = r;
        return c.ntargets++;
    };
    for (int j = 0; j < c.nbands; ++j) {
        if (j > 0 && (c.first_t[j] = add_target(c.start[j])) < 0) return RBL_OK;
        if (j < c.nbands - 1 && (c.last_t[j] = add_target(c.start[j + 1] - 1)) < 0) return RBL_OK;
    }
    for (int t = 1; t < c.ntargets; ++t)
        if (c.target_rank[t] <= c.target_rank[t - 1]) return RBL_OK;   // (cannot happen: bands are disjoint and ordered)
    // clusters: a band of two or more ranks, single-rank bands, the next band of two or more ranks
    int L = 0;
    for (int j = 1; j < c.nbands; ++j) {
        if (size(j) == 1) continue;
        if (c.nclusters == ZB_MAX_CLUSTERS) return RBL_OK;
        bool up = false;
        for (int q = L; q < j; ++q) up = up || c.sigma[q + 1] > c.sigma[q];
        if (j - L > 3) return RBL_OK;   // more than two single-rank bands in a row: left to the sort
        c.cl_L[c.nclusters] = L;
        c.cl_R[c.nclusters] = j;
        c.cl_root[c.nclusters] = up ? 1 : 0;
        ++c.nclusters;
        L = j;
    }
    RBL_TRY(h->mem.alloc(&h->zb.st, (size_t)1));
    RBL_HIP(hipMemsetAsync(h->zb.st, 0, sizeof(ZbState), h->stream));
    RBL_TRY(h->mem.alloc((unsigned char**)&h->zb.hist, zb_hist_bytes()));
    RBL_TRY(h->mem.alloc((unsigned char**)&h->zb.part, zb_partials_bytes()));
    RBL_TRY(h->mem.alloc(&h->zb.tot, (size_t)(4 * ZB_C)));
    RBL_TRY(h->mem.alloc(&h->zb.pack, (size_t)(ZB_GCAP + 1)));
    RBL_TRY(h->mem.pinned(&h->zb.pin, 16, hipHostMallocDefault));
    for (int i = 0; i < 16; ++i) h->zb.pin[i] = 0;
    h->zb.enabled = true;   // set last: the buffers above are all there
    return RBL_OK;
}

// sum_i sigma_i * loss_(i) from n_total values of v (device) -> *out_dev
int risk_from_v(rbl_solver* h, const double* v_all, double* out_dev) {
    hipStream_t s = h->stream;
    if (h->cfg.weight_function == RBL_W_ERM)
        return launch_loss_sum(h->cfg.loss, h->nt, v_all, 1.0 / (double)h->nt, h->partials, out_dev, s, h->rs);
    h->keys_ready = false;   // the sort workspace is reused: keys left by rbl_phase_m are gone
    RBL_TRY(launch_loss_keys(h->nt, v_all, h->sw.keys[0], s, h->rs));   // (own labels: the losses are taken at r * v)
    // piecewise-constant weights: the band sums of the losses need a select, not a sort (zband.hip; exact for any v)
    if (h->zb.enabled)
        return launch_zband_risk(h->cfg.loss, h->zb.cfg, h->nt, h->sw.keys[0], h->zb.st, h->zb.hist, h->zb.part, out_dev, s);
    RBL_TRY(launch_radix_sort(h->sw, h->nt, false, s));
    return launch_sorted_loss_dot(h->cfg.loss, h->nt, h->sw.keys[0], h->sigma_a, h->partials, out_dev, s);
}

}  // namespace

// ================================================================================ C ABI
extern "C" {

int rbl_version(void) { return RBL_VERSION; }

int rbl_sizeof(int which) { return which == 0 ? (int)sizeof(rbl_config) : which == 1 ? (int)sizeof(rbl_stats) : -1; }

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
    h->ld = round_up(cfg->d, 4);
    h->nt = cfg->n_total;
    h->off = cfg->row_offset;
    h->storage = cfg->storage;
    h->esz = cfg->storage == RBL_STORE_F32 ? 4 : 8;
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
    const int64_t n = h->n, ld = h->ld, nt = h->nt;
    if (owner) {
        h->shared = owner->shared;
        h->borrower = true;
        h->D = owner->D;
        h->G = owner->G;
        h->ysign = owner->ysign;
        h->colstats = owner->colstats;
    } else {
        h->shared = std::make_shared<DevArena>();
        const size_t dbytes = (size_t)(n > 0 ? n : 1) * ld * h->esz;
        if (h->shared->alloc((unsigned char**)&h->D, dbytes) != RBL_OK) {
            rbl_set_error("hipMalloc of the %lld x %lld matrix (%zu bytes) failed: %s", (long long)n, (long long)ld, dbytes,
                          hipGetErrorString(hipGetLastError()));
            return RBL_ERR_NOMEM;
        }
        RBL_TRY(h->shared->alloc(&h->ysign, (size_t)n));
        RBL_TRY(h->shared->alloc(&h->colstats, (size_t)ld * 4));
        if (!cfg->objective_only) RBL_TRY(h->shared->alloc(&h->G, (size_t)ld * ld));
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
    if (!cfg->objective_only) {
        size_t gb = owner ? 0 : gram_slab_bytes(ld, h->num_cu, n > 0 ? n : 1);   // (a borrower never forms G)
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
    }
    RBL_TRY(mem.alloc((unsigned char**)&h->slab, h->slab_bytes));
    if (h->sorted_path) {
        RBL_TRY(alloc_sort(mem, h->sw, nt, !cfg->objective_only, h->stream));
        if (!cfg->objective_only) {
            RBL_TRY(alloc_pav(mem, h->pw, nt, h->stream));
            RBL_TRY(mem.alloc(&h->s32.mm, (size_t)s32_range_words()));
            RBL_TRY(mem.alloc(&h->s32.flag, 1));
            RBL_TRY(mem.pinned(&h->s32.pin, 16, hipHostMallocDefault));
            for (int i = 0; i < 16; ++i) h->s32.pin[i] = 0;
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
        const char* nf = getenv("RBL_NO_FUSE");
        h->fused_ok = !h->sorted_path && !(nf && nf[0] == '1') && sweep_erm_supported(h->storage, ld);
        h->fuse_v = !h->fused_ok && !(nf && nf[0] == '1') && n > 0 && sweep_v_supported(h->storage, ld);
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
        // everything rbl_gram_finish derives from G alone
        h->L = owner->L;
        h->ww.eig_Vt = owner->ww.eig_Vt;
        h->ww.eig_V = owner->ww.eig_V;
        h->ww.eig_lambda = owner->ww.eig_lambda;
        h->ww.eig_ok = owner->ww.eig_ok;
        h->eig_sweeps = owner->eig_sweeps;
        h->data_ready = h->gram_local_done = h->gram_ready = true;
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
    if (!owner->data_ready) {
        rbl_set_error("create_shared: the owner has no data yet (rbl_set_data / rbl_generate_synthetic first)");
        return RBL_ERR_STATE;
    }
    if (!cfg->objective_only && (!owner->gram_ready || !owner->G)) {
        rbl_set_error("create_shared: the owner's Gram matrix is not ready (rbl_gram_local + rbl_gram_finish first)");
        return RBL_ERR_STATE;
    }
    RBL_TRY(check_device(nullptr));
    RBL_HIP(hipSetDevice(oc.device));
    RBL_HIP(hipStreamSynchronize(owner->stream));   // D and G are complete before another stream reads them
    rbl_solver* h = new rbl_solver();
    h->cfg = *cfg;
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

int rbl_create(const rbl_config* cfg, rbl_solver** out) {
    if (!out) {
        rbl_set_error("out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = nullptr;
    RBL_TRY(validate(cfg));
    int cnt = 0;
    RBL_TRY(check_device(&cnt));
    if (cfg->device < 0 || cfg->device >= cnt) {
        rbl_set_error("device %d out of range (%d devices)", cfg->device, cnt);
        return RBL_ERR_INVALID;
    }
    RBL_HIP(hipSetDevice(cfg->device));
    rbl_solver* h = new rbl_solver();
    h->cfg = *cfg;
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

// Entry of the functions that advance the iteration (phases, step, solve) or only read handle
// bookkeeping: a speculative w-step in flight stays.
#define RBL_ENTER_ITER(h)                              \
    do {                                               \
        if (!(h)) {                                    \
            rbl_set_error("solver handle is NULL");    \
            return RBL_ERR_INVALID;                    \
        }                                              \
        RBL_HIP(hipSetDevice((h)->cfg.device));        \
    } while (0)

// The sort-free z-step (zband.hip) reports through a pinned word whether it could certify its result.  Whoever is about
// to look at z (or at the q formed from it) before rbl_phase_w has done so settles it here: wait for the word; not
// certified -> the z-step (and q, if rbl_phase_q has run) is redone with the sort + merge-tree PAV, and the fast path
// pauses for 2, 4, ... 64 iterations (the first iterations pool most of the rows in one block; that passes).
// *redone (optional): tells rbl_phase_w that its w-step has to be repeated.
int zb_resolve(rbl_solver* h, bool* redone = nullptr) {
    if (redone) *redone = false;
    if (h->s32.used) {
        // z-step with 32-bit sort keys: a run of equal keys too long for the fix-up (many m within range / 2^32 of each
        // other: ties on a grid, a degenerate range) - redo this iteration's z-step (and q) with 64-bit keys, and stay on
        // them for the next 64 iterations
        h->s32.used = false;
        volatile int* pin = h->s32.pin;
        if (pin[0] != h->s32.seq) rbl_spin_wait(pin, 0, h->stream);
        if (pin[0] != h->s32.seq) {
            rbl_set_error("z-step: the verdict of the 32-bit sort was never written");
            (void)hipGetLastError();
            return RBL_ERR_HIP;
        }
        if (pin[1] != 0) {
            h->s32.skip_until = h->iter + 1 + 64;
            const bool q_done = h->s32.q_done;
            h->s32.q_done = false;
            RBL_TRY(z_step_sorted(h, h->m, h->step_rho, false));
            if (q_done) {
                RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
                RBL_TRY(launch_gemvt(h->storage, h->D, h->n, h->ld, h->c, h->slab, h->q, h->num_cu, h->stream));
                h->nd_launches += 1;
            }
            if (redone) *redone = true;
        }
        return RBL_OK;
    }
    if (!h->zb.used) return RBL_OK;
    h->zb.used = false;
    volatile int* pin = h->zb.pin;
    if (pin[0] != h->zb.seq) rbl_spin_wait(pin, 0, h->stream);
    if (pin[0] != h->zb.seq) {
        rbl_set_error("banded z-step: its status word was never written");
        (void)hipGetLastError();
        return RBL_ERR_HIP;
    }
    if (pin[1] == ZB_OK) {
        h->zb.backoff = 0;
        return RBL_OK;
    }
    h->zb.backoff = h->zb.backoff < 2 ? 2 : (h->zb.backoff >= 32 ? 64 : 2 * h->zb.backoff);
    h->zb.skip_until = h->iter + 1 + h->zb.backoff;
    h->zb.mode = 2;
    const bool q_done = h->zb.q_done;
    h->zb.c_ready = h->zb.q_done = false;
    RBL_TRY(z_step_sorted(h, h->m, h->step_rho, false));
    if (q_done) {
        RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
        RBL_TRY(launch_gemvt(h->storage, h->D, h->n, h->ld, h->c, h->slab, h->q, h->num_cu, h->stream));
        h->nd_launches += 1;
    }
    if (redone) *redone = true;
    return RBL_OK;
}

// w_{k+1} was computed ahead of time (rbl_phase_finish); anything that looks at or replaces the
// state between two iterations must see w_k: put it back (the w-step is simply redone later).
int cancel_spec(rbl_solver* h) {
    if (!h->spec_w) return RBL_OK;
    h->spec_w = false;
    h->spec_timed = false;
    RBL_HIP(hipMemcpyAsync(h->w, h->w_prev, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

// Entry of every other function of the API
#define RBL_ENTER(h)              \
    do {                          \
        RBL_ENTER_ITER(h);        \
        RBL_TRY(zb_resolve(h));   \
        RBL_TRY(cancel_spec(h));  \
    } while (0)

// the data path (upload, generator, Gram matrix) belongs to the handle that owns D and G
#define RBL_NOT_BORROWER(h, what)                                                                             \
    do {                                                                                                      \
        if ((h)->borrower) {                                                                                  \
            rbl_set_error(what ": this handle borrows its data (rbl_create_shared) - call it on the owner");  \
            return RBL_ERR_STATE;                                                                             \
        }                                                                                                     \
    } while (0)

int rbl_set_stream(rbl_solver* h, void* hip_stream) {
    RBL_ENTER(h);
    RBL_HIP(hipStreamSynchronize(h->stream));
    // NULL is a real stream (the legacy default stream torch uses unless told otherwise);
    // (void*)-1 restores the handle's own non-blocking stream
    h->stream = (hip_stream == (void*)-1) ? h->own_stream : (hipStream_t)hip_stream;
    return RBL_OK;
}

int rbl_set_data(rbl_solver* h, const double* X, const double* y, int64_t ldx) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "set_data");
    if (!X || !y || ldx < h->d) {
        rbl_set_error("set_data: bad arguments (ldx=%lld, d=%lld)", (long long)ldx, (long long)h->d);
        return RBL_ERR_INVALID;
    }
    for (int64_t i = 0; i < h->n; ++i) {
        if (!(y[i] == 1.0 || y[i] == -1.0)) {
            rbl_set_error("set_data: labels must be +1/-1 (y[%lld] = %g)", (long long)i, y[i]);
            return RBL_ERR_INVALID;
        }
    }
    const int64_t n = h->n, d = h->d;
    if (n > 0) {
        // The caller's rows are pinned in place for the duration of the call (hipHostRegister), so the
        // 64 MB chunks go over PCIe by DMA at link speed, and two staging buffers let the copy of chunk
        // k+1 run (second stream) while chunk k is converted to the storage type into D.  If the
        // pages cannot be pinned the chunks are copied from pageable memory instead (slower, same result).
        int64_t chunk = (int64_t)((64LL << 20) / (sizeof(double) * (size_t)ldx));
        if (chunk < 1) chunk = 1;
        if (chunk > n) chunk = n;
        const size_t xbytes = sizeof(double) * (size_t)n * (size_t)ldx;
        const bool pinned = hipHostRegister(const_cast<double*>(X), xbytes, hipHostRegisterDefault) == hipSuccess;
        if (!pinned) (void)hipGetLastError();
        int rc = RBL_OK;
        {
            DevArena tmp;   // the staging buffers, freed at the end of this block (after the last stream wait)
            double *Xd[2] = {nullptr, nullptr}, *yd = nullptr;
            hipStream_t copy_stream = nullptr;
            hipEvent_t copied[2] = {nullptr, nullptr}, formed[2] = {nullptr, nullptr};
            auto cleanup = [&]() {
                for (int k = 0; k < 2; ++k) {
                    if (copied[k]) (void)hipEventDestroy(copied[k]);
                    if (formed[k]) (void)hipEventDestroy(formed[k]);
                }
                if (copy_stream) (void)hipStreamDestroy(copy_stream);
                if (pinned) (void)hipHostUnregister(const_cast<double*>(X));
            };
            if (tmp.alloc(&Xd[0], (size_t)chunk * ldx) != RBL_OK || tmp.alloc(&Xd[1], (size_t)chunk * ldx) != RBL_OK ||
                tmp.alloc(&yd, (size_t)n) != RBL_OK) {
                cleanup();
                return RBL_ERR_NOMEM;
            }
            bool ok = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) == hipSuccess;
            for (int k = 0; k < 2 && ok; ++k)
                ok = hipEventCreateWithFlags(&copied[k], hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&formed[k], hipEventDisableTiming) == hipSuccess;
            ok = ok && hipMemcpyAsync(yd, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream) == hipSuccess;
            ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
            if (!ok) {
                rbl_set_error("set_data: stream / event / label upload failed: %s", hipGetErrorString(hipGetLastError()));
                cleanup();
                return RBL_ERR_HIP;
            }
            int64_t k = 0;
            for (int64_t r0 = 0; r0 < n && rc == RBL_OK; r0 += chunk, ++k) {
                const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
                const int b = (int)(k & 1);
                hipError_t e = hipSuccess;
                if (k >= 2) e = hipStreamWaitEvent(copy_stream, formed[b], 0);   // staging buffer b has been consumed
                if (e == hipSuccess)
                    e = hipMemcpyAsync(Xd[b], X + r0 * ldx, sizeof(double) * rows * ldx, hipMemcpyHostToDevice, copy_stream);
                if (e == hipSuccess) e = hipEventRecord(copied[b], copy_stream);
                if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, copied[b], 0);
                if (e != hipSuccess) {
                    rbl_set_error("set_data: upload failed: %s", hipGetErrorString(e));
                    rc = RBL_ERR_HIP;
                    break;
                }
                rc = launch_form_D(h->storage, h->D, h->ld, r0, Xd[b], ldx, yd + r0, rows, d, h->stream);
                if (rc == RBL_OK && hipEventRecord(formed[b], h->stream) != hipSuccess) rc = RBL_ERR_HIP;
            }
            if (hipStreamSynchronize(copy_stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
                if (rc == RBL_OK) {
                    rbl_set_error("set_data: %s", hipGetErrorString(hipGetLastError()));
                    rc = RBL_ERR_HIP;
                }
            }
            cleanup();
        }
        RBL_TRY(rc);
        std::vector<signed char> ys((size_t)n);
        for (int64_t i = 0; i < n; ++i) ys[(size_t)i] = y[i] > 0 ? 1 : -1;
        RBL_HIP(hipMemcpy(h->ysign, ys.data(), (size_t)n, hipMemcpyHostToDevice));
    }
    h->data_ready = true;
    h->gram_ready = h->gram_local_done = false;
    h->v_valid = false;
    return RBL_OK;
}

int rbl_synth_local(rbl_solver* h, uint64_t seed, double class_sep, double flip_y) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "synth_local");
    // positions of the 2 informative + 2 redundant columns, the 2x2 mixing matrix of the redundant ones, the four
    // clusters' covariance matrices A_k (entries uniform in (-1, 1)) and which hypercube vertex each cluster sits on
    // (a random permutation; cluster k belongs to class k % 2) - make_classification's geometry draws - from a small
    // host-side LCG keyed by the seed (identical on every rank)
    uint64_t st = seed * 6364136223846793005ull + 1442695040888963407ull;
    auto next = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(st >> 33);
    };
    int special[4] = {-1, -1, -1, -1};
    const int nspec = h->d >= 4 ? 4 : (int)h->d;
    for (int k = 0; k < nspec; ++k) {
        for (;;) {
            int c = (int)(next() % (uint32_t)h->d);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= special[j] == c;
            if (!dup) {
                special[k] = c;
                break;
            }
        }
    }
    double mix[4];
    for (int k = 0; k < 4; ++k) mix[k] = 2.0 * ((double)next() / 2147483648.0) - 1.0;
    double A16[16];
    for (int k = 0; k < 16; ++k) A16[k] = 2.0 * ((double)next() / 2147483648.0) - 1.0;
    int vertex[4] = {0, 1, 2, 3};
    for (int i = 3; i > 0; --i) {
        const int j = (int)(next() % (uint32_t)(i + 1));
        std::swap(vertex[i], vertex[j]);
    }
    RBL_TRY(launch_synth(h->storage, h->D, h->n, h->ld, h->d, h->off, seed, class_sep, flip_y, special, mix, A16, vertex,
                         h->ysign, h->stream));
    // column sums / sums of squares of the local rows -> colstats[0 .. 2 ld)
    RBL_TRY(launch_colstats(h->storage, h->D, h->n, h->ld, h->slab, h->colstats, h->colstats + h->ld, h->num_cu,
                            h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

int rbl_synth_finish(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "synth_finish");
    // preprocessing.scale (load_data.py:115): (x - mean) / std with the population std
    const int64_t ld = h->ld;
    std::vector<double> st((size_t)ld * 4, 0.0);
    RBL_HIP(hipMemcpy(st.data(), h->colstats, sizeof(double) * ld * 2, hipMemcpyDeviceToHost));
    const double nt = (double)h->nt;
    for (int64_t j = 0; j < ld; ++j) {
        const double mean = st[j] / nt;
        double var = st[ld + j] / nt - mean * mean;
        if (!(var > 0.0)) var = 1.0;
        st[2 * ld + j] = mean;
        st[3 * ld + j] = 1.0 / std::sqrt(var);
    }
    RBL_HIP(hipMemcpy(h->colstats + 2 * ld, st.data() + 2 * ld, sizeof(double) * ld * 2, hipMemcpyHostToDevice));
    RBL_TRY(launch_standardize_negy(h->storage, h->D, h->n, ld, h->d, h->colstats + 2 * ld, h->colstats + 3 * ld,
                                    h->ysign, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    h->data_ready = true;
    h->gram_ready = h->gram_local_done = false;
    h->v_valid = false;
    return RBL_OK;
}

int rbl_generate_synthetic(rbl_solver* h, uint64_t seed, double class_sep, double flip_y) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "generate_synthetic");
    if (h->nt != h->n) {
        rbl_set_error("generate_synthetic: sharded problem - use rbl_synth_local, sum RBL_BUF_COLSTATS, rbl_synth_finish");
        return RBL_ERR_STATE;
    }
    RBL_TRY(rbl_synth_local(h, seed, class_sep, flip_y));
    return rbl_synth_finish(h);
}

int rbl_set_labels(rbl_solver* h, const double* y) {
    RBL_ENTER(h);
    if (!h->borrower) {
        rbl_set_error("set_labels: only a handle that borrows its data (rbl_create_shared) can carry labels of its own");
        return RBL_ERR_STATE;
    }
    if (h->iter > 0) {
        rbl_set_error("set_labels: the handle has iterated already (iter = %lld)", (long long)h->iter);
        return RBL_ERR_STATE;
    }
    if (h->in_group) {
        rbl_set_error("set_labels: the handle is a member of a group - destroy the group first");
        return RBL_ERR_STATE;
    }
    if (h->nt != h->n) {
        rbl_set_error("set_labels: row-sharded handle (n=%lld of %lld) - the distributed z-steps carry no labels of their own",
                      (long long)h->n, (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    if (!y) {
        rbl_set_error("set_labels: y is NULL");
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n;
    for (int64_t i = 0; i < n; ++i)
        if (!(y[i] == 1.0 || y[i] == -1.0)) {
            rbl_set_error("set_labels: labels must be +1/-1 (y[%lld] = %g)", (long long)i, y[i]);
            return RBL_ERR_INVALID;
        }
    RBL_HIP(hipStreamSynchronize(h->stream));
    std::vector<signed char> yo((size_t)n), r((size_t)n), ys((size_t)n);
    RBL_HIP(hipMemcpy(yo.data(), h->ysign, (size_t)n, hipMemcpyDeviceToHost));
    bool differs = false;
    for (int64_t i = 0; i < n; ++i) {
        ys[(size_t)i] = y[i] > 0 ? 1 : -1;
        r[(size_t)i] = (signed char)(ys[(size_t)i] * yo[(size_t)i]);
        differs = differs || r[(size_t)i] < 0;
    }
    if (!differs && !h->rs) return RBL_OK;   // the owner's labels on an ordinary borrower: nothing changes
    // z and lambda move from the sign convention they are stored in to the new one (both start as constants)
    std::vector<double> zh, lh;
    if (h->z) {
        zh.resize((size_t)n);
        lh.resize((size_t)n);
        RBL_HIP(hipMemcpy(zh.data(), h->z, sizeof(double) * n, hipMemcpyDeviceToHost));
        RBL_HIP(hipMemcpy(lh.data(), h->lam, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (h->rs) {
            flip_rows(h, zh.data());
            flip_rows(h, lh.data());
        }
    }
    if (!differs) {   // the owner's labels: an ordinary borrower
        if (h->rs) h->mem.release(h->rs);
        h->rs = nullptr;
        h->rs_host.clear();
        h->ys_host.clear();
    } else {
        if (!h->rs) RBL_TRY(h->mem.alloc(&h->rs, (size_t)n));
        RBL_HIP(hipMemcpy(h->rs, r.data(), (size_t)n, hipMemcpyHostToDevice));
        h->rs_host.swap(r);
        h->ys_host.swap(ys);
    }
    if (h->z) {
        RBL_TRY(upload_rows(h, h->z, zh.data()));
        RBL_TRY(upload_rows(h, h->lam, lh.data()));
    }
    if (!h->cfg.objective_only) {
        // the sign is not part of the single-sweep erm pass' in-pass prox: such a handle runs the two-pass iteration
        const char* nf = getenv("RBL_NO_FUSE");
        h->fused_ok = !h->rs && !h->sorted_path && !(nf && nf[0] == '1') && sweep_erm_supported(h->storage, h->ld);
    }
    h->z_ready = h->p_valid = h->p_pending = h->pred_valid = false;
    h->keys_ready = h->s32.m_ready = false;
    return RBL_OK;
}

// One-vs-rest decision on the rows of `data`: cls[i] = argmax_j x_i . w_j (ties: the lowest j).  D = -y X, so the
// scores are -y_i (D w_j)_i: the multi-column V product of the groups (sweep_multi.hip), ceil(k / k_per_pass) passes
// over D, each followed by the row-wise comparison against the best score so far.
int rbl_decide_multi(rbl_solver* h, int k, const double* W, int32_t* cls) {
    RBL_ENTER(h);
    if (!h->data_ready) {
        rbl_set_error("decide_multi: no data");
        return RBL_ERR_STATE;
    }
    if (k < 1 || k > 64 || !W || !cls) {
        rbl_set_error("decide_multi: 1..64 columns (got %d), W and cls not NULL", k);
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n, ld = h->ld, d = h->d;
    if (n <= 0) return RBL_OK;
    hipStream_t s = h->stream;
    const bool multi = sweep_multi_supported(h->storage, ld);
    const int kpp = multi ? sweep_multi_k(h->storage, ld) : 1;
    DevArena mem;   // scratch of this call, freed on return (after the stream wait)
    double *dw = nullptr, *dv = nullptr, *best = nullptr;
    int* dcls = nullptr;
    std::vector<double> wp((size_t)ld * k, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < d; ++i) wp[(size_t)j * ld + i] = W[(size_t)j * d + i];
    RBL_TRY(mem.alloc(&dw, wp.size()));
    RBL_TRY(mem.alloc(&dv, (size_t)n * kpp));
    RBL_TRY(mem.alloc(&best, (size_t)n));
    RBL_TRY(mem.alloc(&dcls, (size_t)n));
    RBL_HIP(hipMemcpy(dw, wp.data(), sizeof(double) * wp.size(), hipMemcpyHostToDevice));
    int rc = RBL_OK;
    for (int j0 = 0; j0 < k && rc == RBL_OK; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {   // outside the multi-column kernels' widths: the single-column pass per column
            rc = launch_gemv(h->storage, h->D, n, ld, dw + (size_t)j0 * ld, dv, h->num_cu, s);
        } else {
            const double* w[RBL_MULTI_KMAX];
            double* v[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                w[j] = dw + (size_t)(j0 + j) * ld;
                v[j] = dv + (size_t)j * n;
            }
            rc = launch_sweep_v_multi(h->storage, h->D, n, ld, kk, w, nullptr, nullptr, v, nullptr, nullptr, nullptr, h->num_cu, s);
        }
        if (rc == RBL_OK) rc = launch_decide_rows(n, kk, j0, dv, h->ysign, best, dcls, s);
    }
    if (rc == RBL_OK && (hipMemcpyAsync(cls, dcls, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = RBL_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;   // before the scratch goes
    if (rc == RBL_ERR_HIP) rbl_set_error("decide_multi: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

int rbl_get_labels(rbl_solver* h, double* y_out) {
    RBL_ENTER(h);
    if (h->rs) {   // labels of its own (rbl_set_labels)
        for (int64_t i = 0; i < h->n; ++i) y_out[i] = (double)h->ys_host[(size_t)i];
        return RBL_OK;
    }
    std::vector<signed char> t((size_t)h->n);
    RBL_HIP(hipMemcpy(t.data(), h->ysign, (size_t)h->n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < h->n; ++i) y_out[i] = (double)t[i];
    return RBL_OK;
}

int rbl_gram_local(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "gram_local");
    if (!h->data_ready || h->cfg.objective_only) {
        rbl_set_error("gram: no data (or objective-only handle)");
        return RBL_ERR_STATE;
    }
    RBL_TRY(launch_gram(h->storage, h->D, h->n, h->ld, h->d, h->slab, h->G, h->num_cu, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    h->gram_local_done = true;
    h->ww.eig_ok = false;
    return RBL_OK;
}

int rbl_gram_finish(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "gram_finish");
    if (!h->gram_local_done) {
        rbl_set_error("gram_finish before gram_local");
        return RBL_ERR_STATE;
    }
    double lam = 0.0;
    RBL_TRY(launch_power_iteration(h->G, h->ld, h->ww.yk, h->ww.Gy, h->ww.scal, 100, &lam, h->stream));
    h->L = 1.02 * lam;
    if (!(h->L > 0.0)) h->L = 1.0;
    // l2 w-step: RBL_RIDGE_EIG=1 replaces the warm-started CG by a one-time eigendecomposition of G (eig.hip).
    // Opt-in: it makes an iteration 0.13 ms shorter at d = 1000 (14 CG iterations -> 5 small launches) but the
    // Jacobi sweeps cost 0.8 s of setup there - 6000 iterations to break even, and a solve runs a few hundred
    h->ww.eig_ok = false;
    static const bool ridge_eig = [] {
        const char* e = getenv("RBL_RIDGE_EIG");
        return e && e[0] == '1';
    }();
    if (h->cfg.wstep == RBL_WSTEP_L2 && h->ld <= 2048 && ridge_eig) {
        const size_t nn = (size_t)h->ld * (size_t)h->ld;
        if (!h->ww.eig_Vt) {
            double *Vt = nullptr, *V = nullptr, *lambda = nullptr;
            RBL_TRY(h->shared->alloc(&Vt, nn));   // derived from G alone: shared with the borrowers
            RBL_TRY(h->shared->alloc(&V, nn));
            RBL_TRY(h->shared->alloc(&lambda, (size_t)h->ld));
            h->ww.eig_V = V;
            h->ww.eig_lambda = lambda;
            h->ww.eig_Vt = Vt;   // set last: it says the basis buffers are there
        }
        int rc = RBL_OK, sweeps = 0;
        {
            DevArena tmp;   // Jacobi scratch, freed after the stream wait
            double* Bt = nullptr;
            unsigned long long* off = nullptr;
            RBL_TRY(tmp.alloc(&Bt, nn));
            RBL_TRY(tmp.alloc(&off, 1));
            rc = launch_eig_jacobi(h->G, h->ld, h->d, Bt, h->ww.eig_Vt, h->ww.eig_V, h->ww.eig_lambda, off, h->stream, &sweeps);
            (void)hipStreamSynchronize(h->stream);
        }
        RBL_TRY(rc);
        h->ww.eig_ok = sweeps > 0;
        h->eig_sweeps = sweeps;
    }
    h->gram_ready = true;
    return RBL_OK;
}

int rbl_get_D(rbl_solver* h, double* out) {
    RBL_ENTER(h);
    if (!h->data_ready) {
        rbl_set_error("get_D: no data");
        return RBL_ERR_STATE;
    }
    const int64_t n = h->n, d = h->d;
    int64_t chunk = (64LL << 20) / (8 * d);
    if (chunk < 1) chunk = 1;
    DevArena mem;   // the conversion buffer, freed on return
    double* tmp = nullptr;
    RBL_TRY(mem.alloc(&tmp, (size_t)chunk * d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
        RBL_TRY(launch_D_to_f64(h->storage, (const char*)h->D + (size_t)r0 * h->ld * h->esz, h->ld, rows, d, tmp, h->stream));
        if (hipMemcpyAsync(out + r0 * d, tmp, sizeof(double) * rows * d, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return RBL_ERR_HIP;
    }
    if (h->rs)   // -y_k * X = r * (-y_owner * X)
        for (int64_t i = 0; i < n; ++i)
            if (h->rs_host[(size_t)i] < 0)
                for (int64_t j = 0; j < d; ++j) out[i * d + j] = -out[i * d + j];
    return RBL_OK;
}

int rbl_get_state(rbl_solver* h, double* w, double* z, double* lam, double* rho, int64_t* iter, double* smooth_t) {
    RBL_ENTER_ITER(h);
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
        h->v_valid = false;
        h->z_ready = false;
    }
    if (z && h->z) {
        RBL_TRY(upload_rows(h, h->z, z));
        h->z_ready = false;
    }
    if (lam && h->lam) {
        RBL_TRY(upload_rows(h, h->lam, lam));
        h->z_ready = false;
        h->p_valid = h->p_pending = false;
    }
    if (rho) {
        h->rho = *rho;
        h->z_ready = false;
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

// ------------------------------------------------------------------------------- phases
static int require_ready(rbl_solver* h) {
    if (h->cfg.objective_only) {
        rbl_set_error("objective-only handle cannot step");
        return RBL_ERR_STATE;
    }
    if (!h->data_ready) {
        rbl_set_error("step before set_data / generate_synthetic");
        return RBL_ERR_STATE;
    }
    if (!h->gram_ready) {
        if (h->nt != h->n) {
            rbl_set_error("sharded problem: call rbl_gram_local, sum RBL_BUF_G over ranks, rbl_gram_finish first");
            return RBL_ERR_STATE;
        }
        RBL_TRY(rbl_gram_local(h));
        RBL_TRY(rbl_gram_finish(h));
    }
    return RBL_OK;
}

// erm problems run ONE sweep of D per iteration (sweep_erm.hip): the pass of iteration k also
// performs the z-step and the q = D^T c accumulation of iteration k+1.  `z_ready` says that
// z_next / q / zz already hold that work for rho == the predicted rho_{k+1}; the phases below
// then skip it.  A wrong prediction only clears the flag (the unfused kernels redo it).
static inline double* q_pinit(rbl_solver* h) { return h->q + h->ld; }      // D^T lambda (first pass only)
static inline double* q_zz(rbl_solver* h) { return h->q + 2 * h->ld; }     // ||z||^2 of the current z

// kernel events in this iteration?  (every profile_every-th one: an event record costs ~5 us of stream time)
static inline bool prof_now(const rbl_solver* h) { return h->profile && (h->iter % h->profile_every) == 0; }

int rbl_phase_m(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    RBL_TRY(require_ready(h));
    h->step_rho = h->rho;
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[0], h->stream));
    if (h->fused_ok && h->z_ready) return RBL_OK;
    RBL_TRY(ensure_v(h));
    if (h->sorted_path) {
        if (!h->zb.checked) RBL_TRY(zb_setup(h));
        // which z-step will follow on a single handle: the sort-free one (banded weights), else the sort - with 32-bit
        // keys from the second iteration on (iteration 0 starts from equal m: one run) unless a step was not certified
        const bool banded_next = h->zb.enabled && h->nt == h->n && h->iter > 0 && h->iter >= h->zb.skip_until;
        const bool s32 = h->s32.pin && h->nt == h->n && h->n >= 2 && h->iter > 0 &&
                         h->iter >= h->s32.skip_until && !banded_next;
        h->s32.m_ready = false;
        if (s32) {
            // m = D w - lambda/rho (algorithms.py:89) and its range (the 32-bit keys are a fixed-point image on it)
            RBL_TRY(launch_make_m_range(h->n, h->step_rho, h->v, h->lam, h->m, h->s32.mm, h->stream, h->rs));
            h->s32.m_ready = true;
            h->keys_ready = false;
        } else {
            // m and, in the same pass, the 64-bit sort's input for the z-step: keys of m with the GLOBAL row id as
            // payload (single GPU: off = 0; sharded: what rbl_zd_sort_local sorts)
            RBL_TRY(launch_make_m_keys(h->n, h->step_rho, h->v, h->lam, h->m, h->sw.keys[0], h->sw.vals[0], (u32)h->off,
                                       h->stream, h->rs));
            h->keys_ready = true;
        }
    }
    return RBL_OK;
}

int rbl_phase_z(rbl_solver* h, const void* m_all_dev) {
    RBL_ENTER_ITER(h);
    const double rho = h->step_rho;
    if (h->fused_ok && h->z_ready) {
        std::swap(h->z, h->z_next);  // the z-step of this iteration was done by the previous pass
    } else if (!h->sorted_path) {
        RBL_TRY(launch_erm_zc(h->cfg.loss, h->n, h->sigma0, rho, h->v, h->lam, h->m, h->z, h->c, h->stream, h->rs));
        if (h->fused_ok) RBL_TRY(launch_sumsq(h->n, h->z, h->partials, q_zz(h), h->stream));
    } else {
        const double* msrc = (const double*)m_all_dev;
        if (!msrc) {
            if (h->nt != h->n) {
                rbl_set_error("phase_z: sharded rank-weighted problem needs the gathered m vector");
                return RBL_ERR_STATE;
            }
            msrc = h->m;
        }
        if (!h->zb.checked) RBL_TRY(zb_setup(h));
        h->zb.mode = 0;
        // iteration 0 starts from w = 0, lambda = 0: every m is equal, the keys tie across every band edge
        if (h->zb.enabled && h->nt == h->n && h->keys_ready && msrc == h->m && h->iter > 0 && h->iter >= h->zb.skip_until) {
            h->zb.seq = (h->zb.seq & 0x3fffffff) + 1;
            h->zb.pin[0] = 0;
            RBL_TRY(launch_zband(h->cfg.loss, h->zb.cfg, h->n, rho, h->sw.keys[0], h->m, h->z, h->lam, h->c, h->zb.st, h->zb.hist,
                                 h->zb.part, h->zb.pin, h->zb.seq, h->pw.counters, h->stream, h->rs));
            h->zb.used = true;
            h->zb.q_done = false;
            h->zb.c_ready = true;   // the element-wise pass wrote c = z + lambda/rho as well
            h->zb.mode = 1;
        } else {
            h->zb.c_ready = false;
            RBL_TRY(z_step_sorted(h, msrc, rho));
        }
    }
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[1], h->stream));
    return RBL_OK;
}

int rbl_phase_z_external(rbl_solver* h, const double* z) {
    RBL_ENTER(h);   // a w-step enqueued ahead of time was computed for the library's own z: put w_k back
    if (!z) {
        rbl_set_error("phase_z_external: z is NULL");
        return RBL_ERR_INVALID;
    }
    RBL_TRY(rbl_phase_m(h));   // opens the iteration (step_rho); a no-op for what it has computed already
    if (h->rs) {
        RBL_HIP(hipStreamSynchronize(h->stream));
        RBL_TRY(upload_rows(h, h->z, z));   // the caller's z is in the handle's own sign convention
    } else {
        RBL_HIP(hipMemcpyAsync(h->z, z, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    }
    RBL_HIP(hipStreamSynchronize(h->stream));   // the caller's buffer may go away
    rbl_note_host_sync();
    // a z-step the previous single-sweep pass did ahead of time (z_next, q, ||z||^2) is void: the unfused kernels
    // rebuild q in rbl_phase_q; erm keeps c = z + lambda/rho and ||z||^2 next to z (launch_erm_zc), rebuild both
    h->z_ready = false;
    h->keys_ready = false;
    h->zb.used = h->zb.c_ready = false;   // whatever the library's own z-step left behind is void
    h->s32.used = h->s32.m_ready = false;
    h->zb.mode = 0;
    if (!h->sorted_path) {
        RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
        if (h->fused_ok) RBL_TRY(launch_sumsq(h->n, h->z, h->partials, q_zz(h), h->stream));
    }
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[1], h->stream));
    return RBL_OK;
}

int rbl_phase_w_external(rbl_solver* h, const double* w) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zb_resolve(h));   // the caller's w was formed from a z (and q) it could only read through the resolving entries
    if (!w) {
        rbl_set_error("phase_w_external: w is NULL");
        return RBL_ERR_INVALID;
    }
    // w_prev = w_k: while a w-step enqueued ahead of time is in flight w_k already sits in w_prev
    if (!h->spec_w)
        RBL_HIP(hipMemcpyAsync(h->w_prev, h->w, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
    h->spec_w = false;
    h->spec_timed = false;
    RBL_HIP(hipMemsetAsync(h->w, 0, sizeof(double) * h->ld, h->stream));
    RBL_HIP(hipMemcpyAsync(h->w, w, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    rbl_note_host_sync();
    RBL_TRY(launch_w_stats(h->ld, h->w, h->w_prev, h->red2, h->stream));   // dual residual, regulariser terms
    // no rho prediction was made for this w: the dual update runs unfused, and the d-space recurrence for
    // D^T lambda is re-seeded by the next rbl_phase_q
    h->pred_valid = false;
    h->p_valid = h->p_pending = false;
    h->z_ready = false;        // (a caller that skipped rbl_phase_q: nothing of a previous pass is pending any more)
    h->v_valid = false;
    h->inner_iters = 0;
    h->ww.form = -1;
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[3], h->stream));
    return RBL_OK;
}

int rbl_phase_q(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    if (!(h->fused_ok && h->z_ready)) {
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[2], h->stream));
        // rank-weighted problems: the z-step's scatter writes z alone (one random access per row); c = z +
        // lambda/rho (algorithms.py:192) is a streaming pass here.  (Forming it inside the sweep was tried:
        // the per-row division on the sweep's critical path costs 0.9 ms, the streaming pass 30 us.)
        if (h->sorted_path && !h->zb.c_ready) RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
        h->zb.c_ready = false;
        h->zb.q_done = h->zb.used;   // q of an unsettled sort-free z-step (zb_resolve redoes it with the z-step)
        h->s32.q_done = h->s32.used; // ... and of an unsettled 32-bit sort
        RBL_TRY(launch_gemvt(h->storage, h->D, h->n, h->ld, h->c, h->slab, h->q, h->num_cu, h->stream,
                             prof_now(h) ? h->kev[3] : nullptr));
        h->nd_launches += 1;
        if (prof_now(h)) h->kev_pending[1] = h->n > 0;
        if (h->fused_ok && !h->p_valid) {
            // D^T lambda seeds the d-space recurrence used to predict the primal residual
            RBL_TRY(launch_gemvt(h->storage, h->D, h->n, h->ld, h->lam, h->slab, q_pinit(h), h->num_cu, h->stream));
            h->nd_launches += 1;
            h->p_pending = true;
        }
    }
    h->pending_mask = (h->fused_ok && h->z_ready) ? 0 : 1;  // a fused pass' q was already summed with its residuals
    h->z_ready = false;  // consumed: q (and zz) now belong to the iteration in flight
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[2], h->stream));
    return RBL_OK;
}

static int phase_w_body(rbl_solver* h) {
    const bool spec = h->spec_w;   // this w-step (and what follows it) was enqueued by the previous rbl_phase_finish
    h->spec_w = false;
    int wstep = h->cfg.wstep;
    if (!spec && wstep != RBL_WSTEP_L1)   // the lasso kernel saves its warm start itself
        RBL_HIP(hipMemcpyAsync(h->w_prev, h->w, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
    if (h->p_pending) {
        RBL_HIP(hipMemcpyAsync(h->p, q_pinit(h), sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
        h->p_pending = false;
        h->p_valid = true;
    }
    // The lasso's active-set kernel reports its status through pinned memory; the statistics of
    // the new w and the rho prediction are enqueued behind it before the host looks at the
    // status, so the device works through them while the host waits.  Only when the kernel did
    // not converge (FISTA then changes w again) are they enqueued a second time.
    bool fs_pending = spec;
    const bool predict = h->fused_ok && h->p_valid;
    // the active-set lasso kernel leaves G w of its solution in ww.Gy (it needs the gradient for its
    // own optimality test): no d x d product for the rho prediction unless FISTA had to take over
    bool gw_ready = predict && wstep == RBL_WSTEP_L1;
    if (!spec) {
        RBL_TRY(run_wstep(wstep, h->G, h->ld, h->q, h->step_rho, h->cfg.reg, h->smooth_t, h->L, h->cfg.w_tol, 100000,
                          h->w, h->ww, &h->inner_iters, h->stream, &fs_pending, nullptr, h->w_prev, predict));
        // the persistent CG / nonlinear-CG kernels leave G w of their solution in ww.Gy as well
        if (wstep != RBL_WSTEP_L1) gw_ready = predict && h->ww.gw_valid;
    }
    auto after_w = [&]() -> int {
        if (predict) {
            if (!gw_ready) RBL_TRY(launch_symv(h->G, h->ld, h->w, h->ww.Gy, h->stream));
            RBL_TRY(launch_predict_rho(h->ld, h->q, h->p, h->p_alt, h->w, h->w_prev, h->ww.Gy, q_zz(h), h->step_rho,
                                       217.0 * (double)h->d, h->pred, h->red2, h->stream));
        } else {
            RBL_TRY(launch_w_stats(h->ld, h->w, h->w_prev, h->red2, h->stream));
        }
        return RBL_OK;
    };
    if (!spec) RBL_TRY(after_w());
    if (fs_pending) {
        bool fell_back = false;
        RBL_TRY(finish_wstep_l1(h->G, h->ld, h->q, h->step_rho, h->cfg.reg, h->L, h->cfg.w_tol, 100000, h->w, h->ww,
                                &h->inner_iters, h->stream, &fell_back));
        if (fell_back) {
            gw_ready = false;
            RBL_TRY(after_w());
        }
    }
    h->pred_valid = false;
    if (predict) {
        std::swap(h->p, h->p_alt);   // the recurrence's output becomes D^T lambda of the next iteration
        // test hook: RBL_DEBUG_MISPREDICT_EVERY=N corrupts every N-th prediction so that the
        // verification + unfused recomputation path is exercised (tests/test_gpu_solver.py)
        static const int mis_every = [] {
            const char* e = getenv("RBL_DEBUG_MISPREDICT_EVERY");
            return e ? atoi(e) : 0;
        }();
        if (mis_every > 0 && (h->iter % mis_every) == mis_every - 1) {
            const double wrong = h->step_rho * 1.5;
            RBL_HIP(hipMemcpyAsync(h->pred, &wrong, sizeof(double), hipMemcpyHostToDevice, h->stream));
            RBL_HIP(hipStreamSynchronize(h->stream));
        }
        h->pred_valid = true;
    }
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[3], h->stream));
    return RBL_OK;
}

int rbl_phase_w(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    RBL_TRY(phase_w_body(h));
    // the w-step's own host wait is behind us, so the z-step's status word (written milliseconds earlier in stream
    // order) is there already: no extra synchronisation.  Not certified: z and q were redone, the w-step follows
    bool redone = false;
    RBL_TRY(zb_resolve(h, &redone));
    if (!redone) return RBL_OK;
    RBL_HIP(hipMemcpyAsync(h->w, h->w_prev, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
    return phase_w_body(h);
}

int rbl_phase_dual(rbl_solver* h, int want_objective) {
    RBL_ENTER_ITER(h);

    h->fused_ran = false;
    h->fused_v_ran = false;
    h->nd_launches += 1;
    if (h->fused_ok && h->pred_valid) {
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[4], h->stream));
        RBL_TRY(launch_sweep_erm(h->storage, h->cfg.loss, h->D, h->n, h->ld, h->w, h->z, h->lam, h->v, h->z_next,
                                 h->sigma0, h->step_rho, h->pred, h->slab, h->partials, h->q, h->red, q_zz(h),
                                 h->num_cu, h->stream, prof_now(h) ? h->kev[5] : nullptr, want_objective));
        if (prof_now(h)) h->kev_pending[2] = h->n > 0;
        h->fused_ran = true;
        h->v_valid = want_objective != 0;   // without objective logging the pass does not store v (ensure_v recomputes it if a misprediction asks)
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
    } else if (h->fuse_v) {
        // v = D w and the lambda update in one pass (timed as the gemv of the iteration)
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[0], h->stream));
        RBL_TRY(launch_sweep_v(h->storage, h->D, h->n, h->ld, h->w, h->z, h->lam, h->v, h->step_rho, h->partials, h->red,
                               h->num_cu, h->stream, prof_now(h) ? h->kev[1] : nullptr));
        if (prof_now(h)) h->kev_pending[0] = h->n > 0;
        h->v_valid = true;
        h->fused_v_ran = true;
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
    } else {
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[0], h->stream));
        RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w, h->v, h->num_cu, h->stream));
        if (prof_now(h)) {
            RBL_HIP(hipEventRecord(h->kev[1], h->stream));
            h->kev_pending[0] = true;
        }
        h->v_valid = true;
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
        RBL_TRY(launch_dual(h->cfg.loss, h->n, h->step_rho, h->z, h->v, h->lam, h->partials, h->red, h->stream));
    }
    // own labels: k_dual summed the losses at v as the pass left it - the handle's own are at r * v
    if (h->rs && want_objective && !h->sorted_path)
        RBL_TRY(launch_loss_sum(h->cfg.loss, h->n, h->v, 1.0, h->partials, h->red + 1, h->stream, h->rs));
    h->pending_mask = 2 | (h->fused_ran ? 1 : 0);
    h->want_obj = want_objective;
    h->obj_is_risk = false;
    if (want_objective && h->sorted_path && h->nt == h->n) {
        RBL_TRY(risk_from_v(h, h->v, h->red + 1));
        h->obj_is_risk = true;
    }
    return RBL_OK;
}

// One thread gathers the iteration's scalars into the pinned host block: the host then needs a
// single stream wait and no copies (each small device-to-host copy costs ~15 us of stream time).
static __global__ void k_pack_stats(const double* __restrict__ red, const double* __restrict__ red2,
                             const double* __restrict__ pred, const int* __restrict__ branch,
                             const unsigned* __restrict__ counters, int* __restrict__ zd_err,
                             double* __restrict__ hstat, int seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    hstat[9] = 0.0;
    if (zd_err) {          // distributed z-step: a seam search that ran out of rounds (reported, then cleared)
        hstat[9] = (double)zd_err[0];
        zd_err[0] = 0;
    }
    hstat[0] = red[0];
    hstat[1] = red[1];
    hstat[2] = red2[0];
    hstat[3] = red2[1];
    hstat[4] = red2[2];
    hstat[5] = pred ? pred[0] : 0.0;
    hstat[6] = pred ? pred[1] : 0.0;
    hstat[7] = branch ? (double)branch[0] : -1.0;
    hstat[8] = counters ? (double)counters[0] : 0.0;
    hstat[10] = counters ? (double)counters[3] : 0.0;   // persistent upper-level PAV kernel: 1 = it did not complete
    __threadfence_system();
    reinterpret_cast<volatile int*>(hstat + 15)[0] = seq;   // written last: the host polls this word
}

// part: FIN_ALL = the whole phase; a group step (rbl_group_step) enqueues every member's statistics kernel first
// (FIN_ENQUEUE), waits once for the last one - they run in stream order - and then digests each (FIN_DIGEST: no wait).
enum { FIN_ALL = 0, FIN_ENQUEUE = 1, FIN_DIGEST = 2 };
static int phase_finish_part(rbl_solver* h, rbl_stats* out, int part);

int rbl_phase_finish(rbl_solver* h, rbl_stats* out) {
    RBL_ENTER_ITER(h);
    return phase_finish_part(h, out, FIN_ALL);
}

static int phase_finish_part(rbl_solver* h, rbl_stats* out, int part) {
    float spec_ms = 0.f;   // the w-step of THIS iteration ran before its ev[0]: add its time back
    if (h->spec_timed) (void)hipEventElapsedTime(&spec_ms, h->ev_spec[0], h->ev_spec[1]);
    h->spec_timed = false;
    if (h->phase_timing && part != FIN_DIGEST) RBL_HIP(hipEventRecord(h->ev[5], h->stream));
    volatile int* seq_word = reinterpret_cast<volatile int*>(h->hstat + 15);
    const int pack_seq = (int)((h->iter & 0x3fffffff) + 1);
    if (part != FIN_DIGEST) {
        *seq_word = 0;
        hipLaunchKernelGGL(k_pack_stats, dim3(1), dim3(64), 0, h->stream, h->red, h->red2,
                           h->fused_ran ? h->pred : (const double*)nullptr,
                           (h->sorted_path && h->cfg.weight_function == RBL_W_EHRM) ? h->pw.branch : (const int*)nullptr,
                           h->sorted_path ? h->pw.counters : (const unsigned*)nullptr, h->zd_err, h->hstat, pack_seq);
        RBL_HIP(hipGetLastError());
    }
    if (part == FIN_ENQUEUE) return RBL_OK;   // (group members run the two-pass iteration: nothing to enqueue ahead)
    // Single-sweep lasso iterations: everything the next w-step needs is on the device already
    // (q from the pass, rho_{k+1} = pred[0]), so it is enqueued now and runs while the host waits
    // for and digests this iteration's statistics.  If they say "converged" or "rho was
    // mispredicted", w is put back from w_prev below.
    static const bool no_spec = [] {
        const char* e = getenv("RBL_NO_SPECULATE");
        return e && e[0] == '1';
    }();
    const bool try_spec = part == FIN_ALL && h->fused_ran && h->p_valid && h->cfg.wstep == RBL_WSTEP_L1 && !no_spec;
    if (try_spec) {
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev_spec[0], h->stream));
        bool fs_pending = false;
        RBL_TRY(run_wstep(RBL_WSTEP_L1, h->G, h->ld, h->q, 1.0, h->cfg.reg, h->smooth_t, h->L, h->cfg.w_tol, 100000, h->w,
                          h->ww, nullptr, h->stream, &fs_pending, h->pred, h->w_prev, true));   // leaves G w in ww.Gy
        RBL_TRY(launch_predict_rho(h->ld, h->q, h->p, h->p_alt, h->w, h->w_prev, h->ww.Gy, q_zz(h), 0.0,
                                   217.0 * (double)h->d, h->pred, h->red2, h->stream, h->pred));
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev_spec[1], h->stream));
    }
    if (part == FIN_ALL) rbl_spin_wait(seq_word, 0, h->stream);
    if (*seq_word != pack_seq) {
        rbl_set_error("phase_finish: the statistics kernel did not complete");
        (void)hipGetLastError();
        return RBL_ERR_HIP;
    }
    const volatile double* hs = h->hstat;
    const double r[2] = {hs[0], hs[1]}, r2[3] = {hs[2], hs[3], hs[4]}, pr[2] = {hs[5], hs[6]};
    const int br = (int)hs[7];
    const unsigned merges = (unsigned)hs[8];
    if (hs[9] != 0.0) {
        rbl_set_error("distributed z-step: a seam search did not finish within its rounds");
        return RBL_ERR_STATE;
    }
    if (hs[10] != 0.0) {
        rbl_set_error("z-step: the upper-level PAV kernel did not complete (a wait gave up or its fill list overflowed)");
        return RBL_ERR_HIP;
    }
    if (br >= 0) h->pw.ex.spec = br;   // EHRM: the next iteration speculates the branch this one took
    const double primal = std::sqrt(r[0] > 0.0 ? r[0] : 0.0);   // algorithms.py:135
    const double dual = std::sqrt(r2[0] > 0.0 ? r2[0] : 0.0);   // algorithms.py:136
    double objective = NAN;
    if (h->want_obj) {
        // sharded rank-weighted runs: the caller adds rbl_risk_from_v() of the gathered v
        double risk = 0.0;
        if (h->obj_is_risk) risk = r[1];
        else if (!h->sorted_path) risk = r[1] / (double)h->nt;  // erm: sum over ALL ranks of loss / n
        objective = risk;
        if (h->cfg.wstep == RBL_WSTEP_L2) objective += 0.5 * h->cfg.reg * r2[1];   // objective.py:83-84
        else objective += 0.5 * h->cfg.reg * r2[2];                                 // objective.py:85-86
    }
    const bool conv = primal < h->cfg.tol && dual < h->cfg.tol;  // algorithms.py:137
    const int64_t i = h->iter;
    double rho_next = h->rho;
    if (!conv) {
        // algorithms.py:154-157: the only live branch of the schedule
        const double cap = 217.0 * (double)h->d;
        rho_next = h->rho * (primal > 1e-2 ? 1.02 : 1.07);
        if (rho_next > cap) rho_next = cap;
        if (h->cfg.wstep == RBL_WSTEP_SMOOTH_L1 && i >= 17) {
            // algorithms.py:254-255 (python float %, both operands positive)
            double t = h->smooth_t * 0.9;
            if (t < 1e-9) t = 1e-9;
            h->smooth_t = std::fmod(t, std::pow(rho_next, -0.1)) * std::pow((double)i, -0.1);
        }
    }
    int fused = 0, mispred = 0;
    if (h->fused_ran) {
        fused = 1;
        // the pass already did iteration i+1's z-step with the predicted rho: keep it only if the
        // exact residual leads to exactly that rho (same double arithmetic on both sides)
        h->z_ready = !conv && pr[0] == rho_next;
        if (!conv && !h->z_ready) mispred = 1;
        h->n_fused += 1;
        h->n_mispred += mispred;
    }
    h->pred_valid = false;
    if (try_spec) {
        if (!conv && h->z_ready) {
            h->spec_w = true;
            h->spec_timed = h->phase_timing;
        } else {
            RBL_HIP(hipMemcpyAsync(h->w, h->w_prev, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    float ms[5] = {0, 0, 0, 0, 0};
    if (h->phase_timing) {
        (void)hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]);
        (void)hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]);
        (void)hipEventElapsedTime(&ms[2], h->ev[2], h->ev[3]);
        (void)hipEventElapsedTime(&ms[3], h->ev[3], h->ev[4]);
        (void)hipEventElapsedTime(&ms[4], h->ev[0], h->ev[5]);
        ms[2] += spec_ms;
        ms[4] += spec_ms;
    }
    for (int k = 0; k < 3; ++k) {
        if (h->kev_pending[k]) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, h->kev[2 * k], h->kev[2 * k + 1]) == hipSuccess) {
                h->kt_ms[k] += t;
                h->kt_n[k] += 1;
                if (h->kt_samples[k].size() < (size_t)1 << 16) h->kt_samples[k].push_back(t);
            }
            h->kev_pending[k] = false;
        }
    }
    (void)hipGetLastError();
    if (out) {
        out->iter = i + 1;
        out->primal = primal;
        out->dual = dual;
        out->rho = h->rho;
        out->rho_next = rho_next;
        out->objective = objective;
        out->converged = conv ? 1 : 0;
        out->inner_iters = h->inner_iters;
        out->ehrm_branch = br;
        out->pav_merges = h->sorted_path ? (int)merges : -1;
        out->ms_z = ms[0];
        out->ms_q = ms[1];
        out->ms_w = ms[2];
        out->ms_v = ms[3];
        out->ms_total = ms[4];
        out->fused = fused;
        out->mispredicted = mispred;
        out->fused_v = h->fused_v_ran ? 1 : 0;
        out->host_syncs = g_host_syncs;    // stream waits, blocking copies and spins since the last rbl_phase_finish
        out->sort_passes = h->sorted_path ? h->sort_passes : -1;
        out->zband = h->sorted_path ? h->zb.mode : -1;
        out->wstep_form = h->ww.form;
    }
    h->rho = rho_next;
    h->iter = i + 1;
    g_host_syncs = 0;
    h->sort_passes = 0;
    return RBL_OK;
}

int rbl_step(rbl_solver* h, int want_objective, rbl_stats* out) {
    RBL_ENTER_ITER(h);
    if (h->nt != h->n) {
        rbl_set_error("rbl_step: sharded problem - drive the phase API with collectives in between");
        return RBL_ERR_STATE;
    }
    RBL_TRY(rbl_phase_m(h));
    RBL_TRY(rbl_phase_z(h, nullptr));
    RBL_TRY(rbl_phase_q(h));
    RBL_TRY(rbl_phase_w(h));
    RBL_TRY(rbl_phase_dual(h, want_objective));
    return rbl_phase_finish(h, out);
}

int rbl_solve(rbl_solver* h, int max_iter, int want_objective, rbl_stats* last, double* hist_objective,
              double* hist_primal, double* hist_dual, double* hist_rho, double* hist_time_s, int64_t cap) {
    RBL_ENTER(h);
    if (max_iter <= 0) max_iter = h->cfg.max_iter;
    rbl_stats st;
    std::memset(&st, 0, sizeof(st));
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < max_iter; ++it) {
        RBL_TRY(rbl_step(h, want_objective, &st));
        const int64_t k = st.iter - 1;
        if (k >= 0 && k < cap) {
            if (hist_objective) hist_objective[k] = st.objective;
            if (hist_primal) hist_primal[k] = st.primal;
            if (hist_dual) hist_dual[k] = st.dual;
            if (hist_rho) hist_rho[k] = st.rho;
            if (hist_time_s)
                hist_time_s[k] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        if (st.converged) break;
    }
    RBL_TRY(cancel_spec(h));   // a solve ends on w_k, not on the w-step enqueued ahead of iteration k+1
    if (last) *last = st;
    return RBL_OK;
}

int rbl_finalize_smooth(rbl_solver* h) {
    RBL_ENTER(h);
    if (h->cfg.wstep != RBL_WSTEP_SMOOTH_L1) return RBL_OK;
    RBL_TRY(launch_soft_threshold(h->ld, h->w, h->smooth_t, h->stream));
    h->v_valid = false;
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

int rbl_objective(rbl_solver* h, const double* w, int include_reg, double* out) {
    RBL_ENTER(h);
    if (!h->data_ready || !w || !out) {
        rbl_set_error("objective: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    if (h->nt != h->n) {
        rbl_set_error("objective: sharded handle - use the phase API");
        return RBL_ERR_STATE;
    }
    RBL_HIP(hipMemcpyAsync(h->w_tmp, w, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
    RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w_tmp, h->m, h->num_cu, h->stream));
    RBL_TRY(risk_from_v(h, h->m, h->red2 + 4));
    RBL_TRY(launch_reg_terms(h->ld, h->w_tmp, h->red2 + 5, h->stream));
    double r[3];
    RBL_HIP(hipMemcpyAsync(r, h->red2 + 4, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    double val = r[0];
    if (include_reg && h->cfg.reg > 0.0) {
        if (h->cfg.wstep == RBL_WSTEP_L2) val += 0.5 * h->cfg.reg * r[1];
        else val += 0.5 * h->cfg.reg * r[2];
    }
    *out = val;
    return RBL_OK;
}

// fraction of correctly classified rows of this handle's data (src/util/calculate_acc.py:3-19)
int rbl_accuracy(rbl_solver* h, const double* w, double threshold, double* out) {
    RBL_ENTER(h);
    if (!h->data_ready || !w || !out) {
        rbl_set_error("accuracy: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    if (!(threshold > 0.0 && threshold < 1.0)) {
        rbl_set_error("accuracy: threshold must be in (0, 1)");
        return RBL_ERR_INVALID;
    }
    RBL_HIP(hipMemcpyAsync(h->w_tmp, w, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
    RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w_tmp, h->m, h->num_cu, h->stream));
    RBL_TRY(launch_accuracy(h->cfg.loss, h->n, h->m, h->ysign, std::log(threshold / (1.0 - threshold)), h->partials,
                            h->red2 + 4, h->stream, h->rs));
    double cnt = 0.0;
    RBL_HIP(hipMemcpyAsync(&cnt, h->red2 + 4, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    *out = h->n > 0 ? cnt / (double)h->n : 0.0;   // local rows; sharded callers average by n
    return RBL_OK;
}


// ================================================================== distributed z-step
// Rank-weighted problems on several GPUs: the driver (dist.py: _z_distributed)
// calls these between its collectives; oracle/zdist.py restates every step on the CPU.
// Layout of RBL_BUF_ZD_SMALL (doubles): [0,256) samples | [256,259) bounds | [260,262) EHRM
// fvals | [320,384) candidates | [512, 512+3*4096) partial sums | [12800+..) seam sums.
namespace {
constexpr int ZD_SMALL_DOUBLES = 16384;
constexpr int ZD_OFF_SAMPLES = 0, ZD_OFF_BOUNDS = 256, ZD_OFF_FV = 260, ZD_OFF_CAND = 320, ZD_OFF_PART = 512,
              ZD_OFF_SUMS = 512 + 3 * 4096;
constexpr int ZD_MAX_CAND = 4096;   // world * K

int zd_ensure(rbl_solver* h) {
    if (h->zd_small) return RBL_OK;
    if (!h->sorted_path || h->cfg.objective_only) {
        rbl_set_error("distributed z-step: only for rank-weighted solver handles");
        return RBL_ERR_STATE;
    }
    DevArena& mem = h->mem;
    double* small = nullptr;
    RBL_TRY(mem.alloc(&small, ZD_SMALL_DOUBLES));
    RBL_TRY(mem.alloc(&h->zd_seam, 1));
    RBL_TRY(mem.alloc(&h->zd_err, 1));
    RBL_TRY(mem.alloc(&h->zd_bounds_dev, 80));
    RBL_TRY(mem.alloc(&h->zd_counts_dev, 64));
    RBL_TRY(mem.alloc(&h->zd_zids, (size_t)h->n));
    RBL_TRY(alloc_prefix(mem, h->zd_a, h->nt));
    h->zd_b = h->zd_a;
    if (h->cfg.weight_function == RBL_W_EHRM) RBL_TRY(alloc_prefix(mem, h->zd_b, h->nt));
    RBL_HIP(hipMemsetAsync(h->zd_err, 0, sizeof(int), h->stream));
    h->zd_small = small;   // set last: it says the group is there
    return RBL_OK;
}
}  // namespace

int rbl_zd_sort_local(rbl_solver* h, int nsamples) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nsamples < 1 || nsamples > 256) {
        rbl_set_error("zd_sort_local: 1..256 samples");
        return RBL_ERR_INVALID;
    }
    hipStream_t s = h->stream;
    // keys of the local m, payload = GLOBAL row id
    if (!h->keys_ready) {
        RBL_TRY(launch_keys_from_m(h->n, h->m, h->sw.keys[0], h->sw.vals[0], s));
        if (h->off != 0) RBL_TRY(launch_add_u32(h->n, h->sw.vals[0], (u32)h->off, s));
    }
    h->keys_ready = false;
    RBL_TRY(launch_radix_sort(h->sw, h->n, true, s));
    RBL_TRY(launch_zd_sample(h->sw.keys[0], h->n, nsamples, h->zd_small + ZD_OFF_SAMPLES, s));
    return RBL_OK;
}

// the logged objective of rank weights, sum_i sigma_i loss_(i) (objective.py:73-82), needs the global
// order of the per-sample losses: same sample sort, keys only
int rbl_zd_sort_losses(rbl_solver* h, int nsamples) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nsamples < 1 || nsamples > 256) {
        rbl_set_error("zd_sort_losses: 1..256 samples");
        return RBL_ERR_INVALID;
    }
    hipStream_t s = h->stream;
    RBL_TRY(ensure_v(h));
    h->keys_ready = false;
    RBL_TRY(launch_loss_keys(h->n, h->v, h->sw.keys[0], s));
    RBL_TRY(launch_radix_sort(h->sw, h->n, false, s));
    RBL_TRY(launch_zd_sample(h->sw.keys[0], h->n, nsamples, h->zd_small + ZD_OFF_SAMPLES, s));
    return RBL_OK;
}

// received loss keys in RBL_BUF_ZD_RKEYS: this chunk's share of the risk -> ZD_SMALL[264]
int rbl_zd_risk(rbl_solver* h, int64_t nrecv, int64_t sigma_off) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nrecv < 0 || sigma_off < 0 || sigma_off + nrecv > h->nt) {
        rbl_set_error("zd_risk: chunk [%lld, %lld) outside the %lld sorted positions", (long long)sigma_off,
                      (long long)(sigma_off + nrecv), (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    hipStream_t s = h->stream;
    double* out = h->zd_small + ZD_OFF_FV + 4;
    if (nrecv == 0) {
        RBL_HIP(hipMemsetAsync(out, 0, sizeof(double), s));
        return RBL_OK;
    }
    RBL_HIP(hipMemcpyAsync(h->sw.keys[0], h->sw.keys[1], sizeof(u64) * (size_t)nrecv, hipMemcpyDeviceToDevice, s));
    RBL_TRY(launch_radix_sort(h->sw, nrecv, false, s));
    return launch_sorted_loss_dot(h->cfg.loss, nrecv, h->sw.keys[0], h->sigma_a + sigma_off, h->partials, out, s);
}

int rbl_zd_partition(rbl_solver* h, const void* splitters_dev, int nparts, int64_t* send_counts) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nparts < 1 || nparts > 64) return RBL_ERR_INVALID;
    if (nparts > 1)
        RBL_TRY(launch_zd_split_bounds(h->sw.keys[0], h->n, (const double*)splitters_dev, nparts - 1, h->zd_bounds_dev,
                                       h->stream));
    // the counts stay on the device (RBL_BUF_ZD_COUNTS): the driver all-gathers them there and reads the whole
    // count matrix with ONE host wait; send_counts != NULL additionally downloads this rank's row
    RBL_TRY(launch_zd_counts_from_bounds(h->zd_bounds_dev, nparts, h->n, h->zd_counts_dev, h->stream));
    h->zd_world = nparts;
    if (send_counts) {
        long long hc[64];
        RBL_HIP(hipMemcpyAsync(hc, h->zd_counts_dev, sizeof(long long) * nparts, hipMemcpyDeviceToHost, h->stream));
        RBL_HIP(hipStreamSynchronize(h->stream));
        rbl_note_host_sync();
        for (int j = 0; j < nparts; ++j) send_counts[j] = hc[j];
    }
    return RBL_OK;
}

// the received (key, id) pairs are in RBL_BUF_ZD_RKEYS / RIDS: sort the chunk, sorted m, prefix
// sums of m and of the chunk's slice of sigma; EHRM: this chunk's two singleton-stage sums
int rbl_zd_prepare(rbl_solver* h, int64_t nrecv, int64_t sigma_off) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nrecv < 0 || sigma_off < 0 || sigma_off + nrecv > h->nt) {
        rbl_set_error("zd_prepare: chunk [%lld, %lld) outside the %lld sorted positions", (long long)sigma_off,
                      (long long)(sigma_off + nrecv), (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    hipStream_t s = h->stream;
    // the received pairs move to the sort's input buffers (the pointers behind the typed views stay put)
    RBL_HIP(hipMemcpyAsync(h->sw.keys[0], h->sw.keys[1], sizeof(u64) * (size_t)nrecv, hipMemcpyDeviceToDevice, s));
    RBL_HIP(hipMemcpyAsync(h->sw.vals[0], h->sw.vals[1], sizeof(u32) * (size_t)nrecv, hipMemcpyDeviceToDevice, s));
    h->zd_n = nrecv;
    h->zd_off = sigma_off;
    RBL_TRY(launch_radix_sort(h->sw, nrecv, true, s));   // runs arrive in rank order: stable => ties in row order
    RBL_TRY(launch_unflip_prefix(h->sw.keys[0], nrecv, h->pw.ms, h->pw.pm, s));
    RBL_TRY(launch_prefix(h->sigma_a + sigma_off, nrecv, h->zd_a, s));
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    double* fv = h->zd_small + ZD_OFF_FV;
    if (ehrm) {
        RBL_TRY(launch_prefix(h->sigma_b + sigma_off, nrecv, h->zd_b, s));
        RBL_TRY(launch_ehrm_fvals(nrecv, h->sigma_a + sigma_off, h->sigma_b + sigma_off, h->cfg.B, h->step_rho, h->pw.ms,
                                  h->pw.partials, fv, s, h->pw.u, (double*)h->sw.keys[1]));
    } else {
        RBL_HIP(hipMemsetAsync(fv, 0, 2 * sizeof(double), s));
    }
    return RBL_OK;
}

int rbl_zd_pav(rbl_solver* h, const void* fvals_total_dev) {
    RBL_ENTER_ITER(h);
    hipStream_t s = h->stream;
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    if (ehrm) RBL_TRY(launch_ehrm_pick((const double*)fvals_total_dev, h->pw.branch, s));
    PavExtras ex = h->pw.ex;      // the chunk's upper levels in one launch; the branch comes from the sums over ALL ranks
    ex.num_cu = h->num_cu;
    ex.fpart = nullptr;
    RBL_TRY(launch_pav_tree(h->cfg.loss, h->zd_n, h->step_rho, h->pw.ms, h->sigma_a + h->zd_off, h->sigma_b + h->zd_off,
                            h->pw.u, h->zd_a.view(), h->zd_b.view(), h->pw.pm.view(), ehrm ? h->pw.branch : nullptr, h->pw.recs,
                            h->pw.counters, s,
                            ehrm ? h->pw.u : nullptr, ehrm ? (const double*)h->sw.keys[1] : nullptr, &ex));
    h->pw.ex.bar_parity = ex.bar_parity;
    return RBL_OK;
}

int rbl_zd_bounds(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    return launch_zd_bounds(h->pw.u, h->zd_n, h->zd_small + ZD_OFF_BOUNDS, h->stream);
}

int rbl_zd_seam_setup(rbl_solver* h, int rank, int world, int level, const void* bounds_all_dev) {
    RBL_ENTER_ITER(h);
    if (world < 1 || world > 64 || rank < 0 || rank >= world || level < 1) return RBL_ERR_INVALID;
    h->zd_world = world;
    return launch_zd_seam_setup(rank, world, level, (const double*)bounds_all_dev, h->zd_n, h->zd_seam, h->stream);
}

int rbl_zd_seam_propose(rbl_solver* h, int K, const void* cand_all_prev, const void* part_sum_prev) {
    RBL_ENTER_ITER(h);
    if (K < 1 || K > 64 || K * h->zd_world > ZD_MAX_CAND) return RBL_ERR_INVALID;
    return launch_zd_update_propose(h->cfg.loss, h->zd_seam, h->pw.u, K, h->zd_world, (const double*)cand_all_prev,
                                    (const double*)part_sum_prev, h->step_rho, h->zd_small + ZD_OFF_CAND, h->stream);
}

int rbl_zd_seam_eval(rbl_solver* h, int K, const void* cand_all_dev) {
    RBL_ENTER_ITER(h);
    if (K < 1 || K > 64 || K * h->zd_world > ZD_MAX_CAND) return RBL_ERR_INVALID;
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    return launch_zd_eval(h->zd_seam, h->pw.u, h->zd_a.view(), h->zd_b.view(), h->pw.pm.view(), ehrm ? h->pw.branch : nullptr, K,
                          h->zd_world,
                          (const double*)cand_all_dev, h->zd_small + ZD_OFF_PART, h->stream);
}

int rbl_zd_seam_sums(rbl_solver* h, int K, const void* cand_all_prev, const void* part_sum_prev, int nseams) {
    RBL_ENTER_ITER(h);
    if (nseams < 1 || nseams > 32) return RBL_ERR_INVALID;
    RBL_TRY(launch_zd_update_propose(h->cfg.loss, h->zd_seam, h->pw.u, K, h->zd_world, (const double*)cand_all_prev,
                                     (const double*)part_sum_prev, h->step_rho, nullptr, h->stream));
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    return launch_zd_pooled(h->zd_seam, h->zd_a.view(), h->zd_b.view(), h->pw.pm.view(), ehrm ? h->pw.branch : nullptr, nseams,
                            h->zd_small + ZD_OFF_SUMS, h->zd_err, h->stream);
}

int rbl_zd_seam_fill(rbl_solver* h, const void* sums_total_dev) {
    RBL_ENTER_ITER(h);
    return launch_zd_fill(h->cfg.loss, h->zd_seam, (const double*)sums_total_dev, h->step_rho, h->pw.u, h->zd_n, h->stream);
}

// sort the chunk's (row id, u) by row id: contiguous per owner rank (rows are sharded in
// blocks of nmax); counts[r] = how many go back to rank r.  RBL_BUF_ZD_BIDS / BU hold them.
int rbl_zd_return_partition(rbl_solver* h, int64_t nmax, int world, int64_t* counts) {
    RBL_ENTER_ITER(h);
    if (world < 1 || world > 64 || nmax < 1) return RBL_ERR_INVALID;
    hipStream_t s = h->stream;
    RBL_TRY(launch_zd_ids_to_keys(h->zd_n, h->sw.vals[0], h->sw.keys[0], h->sw.vals[0], s));
    int id_bits = 1;
    while (id_bits < 32 && (1LL << id_bits) < h->nt) ++id_bits;
    RBL_TRY(launch_radix_sort(h->sw, h->zd_n, true, s, id_bits));   // row ids < n_total: 4 passes up to 2^32 rows
    RBL_TRY(launch_zd_gather_back(h->zd_n, h->sw.keys[0], h->sw.vals[0], h->pw.u, h->sw.vals[1], (double*)h->sw.keys[1], s));
    // counts == NULL: no host wait.  How many rows go back to owner r is known to the driver already: it is what
    // r sent to this chunk in the forward exchange (the count matrix of the return trip is the transpose);
    // a seam search that did not finish is reported by rbl_phase_finish (the flag travels in the statistics block)
    if (!counts) return RBL_OK;
    int herr = 0;
    RBL_TRY(launch_zd_owner_bounds(h->sw.keys[0], h->zd_n, nmax, world, h->zd_bounds_dev, s));
    long long hb[65];
    RBL_HIP(hipMemcpyAsync(hb, h->zd_bounds_dev, sizeof(long long) * (world + 1), hipMemcpyDeviceToHost, s));
    RBL_HIP(hipMemcpyAsync(&herr, h->zd_err, sizeof(int), hipMemcpyDeviceToHost, s));
    RBL_HIP(hipStreamSynchronize(s));
    rbl_note_host_sync();
    if (herr) {
        RBL_HIP(hipMemsetAsync(h->zd_err, 0, sizeof(int), s));
        rbl_set_error("distributed z-step: a seam search did not finish within its rounds");
        return RBL_ERR_STATE;
    }
    for (int r = 0; r < world; ++r) counts[r] = hb[r + 1] - hb[r];
    return RBL_OK;
}

// rows received back in RBL_BUF_ZD_ZIDS / ZU: z, c = z + lambda/rho (algorithms.py:103-104, :192)
int rbl_zd_scatter(rbl_solver* h, int64_t n_back) {
    RBL_ENTER_ITER(h);
    if (n_back != h->n) {
        rbl_set_error("zd_scatter: %lld rows came back, %lld are local", (long long)n_back, (long long)h->n);
        return RBL_ERR_STATE;
    }
    const bool ehrm = h->cfg.weight_function == RBL_W_EHRM;
    RBL_TRY(launch_zd_scatter(n_back, h->zd_zids, h->m, ehrm ? h->pw.branch : nullptr, h->cfg.B, ehrm ? 1 : 0, h->step_rho,
                              h->lam, h->z, nullptr, h->off, h->n, h->stream));
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[1], h->stream));
    return RBL_OK;
}

// ---- sort-free z-step for banded rank weights, sharded rows (zband.hip step by step; the driver sums / gathers in between)
static int zbd_ready(rbl_solver* h) {
    if (!h->zb.enabled || !h->keys_ready) {
        rbl_set_error("rbl_zbd_*: call rbl_phase_m and rbl_zbd_begin (applicable) first");
        return RBL_ERR_STATE;
    }
    return RBL_OK;
}
int rbl_zbd_begin(rbl_solver* h, int* applicable, int* root_clusters) {
    RBL_ENTER_ITER(h);
    if (applicable) *applicable = 0;
    if (root_clusters) *root_clusters = 0;
    if (!h->sorted_path) return RBL_OK;
    if (!h->zb.checked) RBL_TRY(zb_setup(h));
    h->zb.mode = 0;
    // iteration 0 (every m equal) and the pause after an uncertified z-step: the caller takes the sort path
    if (!(h->zb.enabled && h->keys_ready && h->iter > 0 && h->iter >= h->zb.skip_until)) return RBL_OK;
    RBL_TRY(launch_zbd_init(h->zb.cfg, h->zb.st, h->zb.hist, h->stream));
    if (applicable) *applicable = 1;
    if (root_clusters) {
        int mask = 0;
        for (int k = 0; k < h->zb.cfg.nclusters; ++k) mask |= h->zb.cfg.cl_root[k] ? (1 << k) : 0;
        *root_clusters = mask;   // bit k: cluster k can pool (rbl_zbd_eval / decide / gather / finish run for it)
    }
    return RBL_OK;
}
int rbl_zbd_hist(rbl_solver* h, int pass) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    return launch_zbd_hist(h->n, h->sw.keys[0], h->zb.st, h->zb.hist, pass, h->stream);
}
int rbl_zbd_scan(rbl_solver* h, int pass) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    return launch_zbd_scan(h->cfg.loss, h->zb.cfg, h->zb.st, h->zb.hist, pass, h->step_rho, h->stream);
}
int rbl_zbd_eval(rbl_solver* h, int k) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    return launch_zbd_eval(h->cfg.loss, h->zb.cfg, h->n, h->sw.keys[0], h->zb.st, k, h->step_rho, h->zb.part, h->zb.tot, h->stream);
}
int rbl_zbd_decide(rbl_solver* h, int k, int last, int* settled) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    if (!settled) return launch_zbd_decide(h->cfg.loss, h->zb.cfg, h->zb.st, k, h->step_rho, h->zb.tot, last, h->stream);
    // the verdict of this pass through pinned memory (one host wait): every rank reads the same answer, the driver stops
    // issuing root passes (and their all-reduces) for this cluster after the pass that settles it
    volatile int* pin = h->zb.pin + 4;
    h->zb.dseq = (h->zb.dseq & 0x3fffffff) + 1;
    pin[0] = 0;
    RBL_TRY(launch_zbd_decide(h->cfg.loss, h->zb.cfg, h->zb.st, k, h->step_rho, h->zb.tot, last, h->stream, h->zb.pin + 4,
                              h->zb.dseq));
    rbl_spin_wait(pin, 0, h->stream);
    if (pin[0] != h->zb.dseq) {
        rbl_set_error("zbd_decide: the verdict of the root pass was never written");
        (void)hipGetLastError();
        return RBL_ERR_HIP;
    }
    *settled = pin[1];
    return RBL_OK;
}
int rbl_zbd_root_passes(void) { return ZB_ROOT_PASSES; }
int rbl_zbd_gather(rbl_solver* h, int k) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    return launch_zbd_gather(h->cfg.loss, h->zb.cfg, h->n, h->sw.keys[0], h->zb.st, k, h->step_rho, h->zb.part, h->zb.pack, h->stream);
}
int rbl_zbd_finish(rbl_solver* h, int k, const void* packs_all_dev, int world) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    if (!packs_all_dev || world < 1 || world > 64) return RBL_ERR_INVALID;
    return launch_zbd_finish(h->cfg.loss, h->zb.cfg, h->zb.st, k, h->step_rho, h->zb.part, (const double*)packs_all_dev, world,
                             h->stream);
}
int rbl_zbd_apply(rbl_solver* h, int* status) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zbd_ready(h));
    h->zb.seq = (h->zb.seq & 0x3fffffff) + 1;
    h->zb.pin[0] = 0;
    RBL_TRY(launch_zbd_apply(h->cfg.loss, h->zb.cfg, h->n, h->step_rho, h->m, h->z, h->lam, h->c, h->zb.st, h->zb.pin, h->zb.seq,
                             h->pw.counters, h->stream));
    // every rank holds the same state, so every rank reads the same verdict and takes the same branch afterwards
    volatile int* pin = h->zb.pin;
    rbl_spin_wait(pin, 0, h->stream);
    if (pin[0] != h->zb.seq) {
        rbl_set_error("banded z-step: its status word was never written");
        (void)hipGetLastError();
        return RBL_ERR_HIP;
    }
    if (status) *status = pin[1];
    if (pin[1] == ZB_OK) {
        h->zb.backoff = 0;
        h->zb.c_ready = true;
        h->zb.mode = 1;
        h->keys_ready = false;
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[1], h->stream));
    } else {
        h->zb.backoff = h->zb.backoff < 2 ? 2 : (h->zb.backoff >= 32 ? 64 : 2 * h->zb.backoff);
        h->zb.skip_until = h->iter + 1 + h->zb.backoff;
        h->zb.mode = 2;   // the caller runs the sort-based distributed z-step (rbl_zd_*) for this iteration
    }
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
        case RBL_BUF_G: p = h->G; cnt = h->ld * h->ld; break;
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

// risk (sum sigma_i loss_(i)) of n_total values of v on the device -> host double
int rbl_risk_from_v(rbl_solver* h, const void* v_all_dev, double* out) {
    RBL_ENTER(h);
    RBL_TRY(risk_from_v(h, (const double*)v_all_dev, h->red2 + 4));
    RBL_HIP(hipMemcpyAsync(out, h->red2 + 4, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    rbl_note_host_sync();
    return RBL_OK;
}

int rbl_kernel_time(rbl_solver* h, int which, double* total_ms, int64_t* launches) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
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

// SPD, DI, EOD, AOD, TI, FNRD of the linear classifier on this handle's rows
// (src/util/fair_metric.py:3-41); group: n doubles with values 0 / 1
int rbl_profile_sampling(rbl_solver* h, int every) {
    RBL_ENTER_ITER(h);   // bookkeeping only: a w-step in flight stays
    if (every < 1) {
        rbl_set_error("profile_sampling: every must be >= 1");
        return RBL_ERR_INVALID;
    }
    h->profile_every = every;
    return RBL_OK;
}

int rbl_fair_statistics(rbl_solver* h, const double* w, const double* group, double threshold, double* out6) {
    RBL_ENTER(h);
    if (!h->data_ready || !w || !group || !out6) {
        rbl_set_error("fair_statistics: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    double c[14];
    {
        DevArena mem;   // the group vector, freed after the readback
        double* gd = nullptr;
        RBL_TRY(mem.alloc(&gd, (size_t)h->n));
        if (hipMemcpyAsync(gd, group, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(h->w_tmp, w, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rbl_set_error("fair_statistics: upload failed");
            return RBL_ERR_HIP;
        }
        RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w_tmp, h->m, h->num_cu, h->stream));
        double* out14 = h->slab;  // scratch (>= 14 doubles)
        RBL_TRY(launch_fair_counts(h->n, h->m, h->ysign, gd, threshold, h->partials, out14, h->stream, h->rs));
        if (hipMemcpyAsync(c, out14, sizeof(double) * 14, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            rbl_set_error("fair_statistics: readback failed");
            return RBL_ERR_HIP;
        }
    }
    // fair_metric.py:11-41, group 0 = G1, group 1 = G2
    const double G1P = c[1] / c[0], G2P = c[7] / c[6];
    const double G1TP = c[2], G1FN = c[3], G1TN = c[4], G1FP = c[5];
    const double G2TP = c[8], G2FN = c[9], G2TN = c[10], G2FP = c[11];
    const double SPD = G2P - G1P;
    const double DI = (G1P == 0.0) ? INFINITY : G2P / G1P;
    const double TPRG1 = G1TP / (G1TP + G1FN), TPRG2 = G2TP / (G2TP + G2FN);
    const double FPRG1 = G1FP / (G1FP + G1TN), FPRG2 = G2FP / (G2FP + G2TN);
    const double FNRG1 = G1FN / (G1TP + G1FN), FNRG2 = G2FN / (G2TP + G2FN);
    const double EOD = TPRG2 - TPRG1;
    const double AOD = 0.5 * (FPRG2 - FPRG1 + EOD);
    const double nn = (double)h->n;
    const double mu = c[12] / nn;
    const double TI = (c[13] - std::log(mu) * c[12]) / mu / nn;  // sum (b/mu) log(b/mu) / n
    out6[0] = SPD;
    out6[1] = DI;
    out6[2] = EOD;
    out6[3] = AOD;
    out6[4] = TI;
    out6[5] = FNRG2 - FNRG1;
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

// ======================================================================== groups: K problems on one D
// One ADMM iteration of every live member per rbl_group_step, the two n x d passes shared (sweep_multi.hip).
struct rbl_group {
    DevArena mem;
    std::vector<rbl_solver*> m;
    std::vector<char> live, saved_fused;
    std::vector<hipStream_t> saved_stream;
    std::vector<int64_t> base_launches;
    std::vector<rbl_stats> last;
    std::vector<int> syncs;          // host waits of each member's own calls in the step in flight
    hipStream_t stream = nullptr;    // every member runs on it while the group exists: one order for all launches
    int device = 0, kpp = 1;
    bool shared_passes = false;      // the width is in the multi-column kernels' range
    double* slab = nullptr;
    int64_t shared_v = 0, shared_q = 0;
};

namespace {
// runs a member's own calls and books the host waits they made on that member
struct SyncBook {
    int& slot;
    int s0;
    explicit SyncBook(int& sl) : slot(sl), s0(g_host_syncs) {}
    ~SyncBook() { slot += g_host_syncs - s0; }
};
}  // namespace

extern "C" {

int rbl_group_create(rbl_solver* const* members, int k, rbl_group** out) {
    if (!out) {
        rbl_set_error("group_create: out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = nullptr;
    if (!members || k < 1 || k > 64) {
        rbl_set_error("group_create: 1..64 members (got %d)", k);
        return RBL_ERR_INVALID;
    }
    for (int i = 0; i < k; ++i) {
        rbl_solver* h = members[i];
        if (!h) {
            rbl_set_error("group_create: member %d is NULL", i);
            return RBL_ERR_INVALID;
        }
        for (int j = 0; j < i; ++j)
            if (members[j] == h) {
                rbl_set_error("group_create: member %d is listed twice", i);
                return RBL_ERR_INVALID;
            }
        if (h->in_group) {
            rbl_set_error("group_create: member %d already belongs to a group", i);
            return RBL_ERR_INVALID;
        }
        if (h->shared != members[0]->shared || h->D != members[0]->D) {
            rbl_set_error("group_create: member %d does not share member 0's data (rbl_create_shared)", i);
            return RBL_ERR_INVALID;
        }
        if (h->nt != h->n) {
            rbl_set_error("group_create: member %d is a row shard (n=%lld of %lld): groups are single-process problems", i,
                          (long long)h->n, (long long)h->nt);
            return RBL_ERR_INVALID;
        }
        if (h->cfg.objective_only) {
            rbl_set_error("group_create: member %d is an objective-only handle", i);
            return RBL_ERR_INVALID;
        }
    }
    rbl_solver* h0 = members[0];
    RBL_HIP(hipSetDevice(h0->cfg.device));
    for (int i = 0; i < k; ++i) {
        RBL_TRY(require_ready(members[i]));
        RBL_TRY(zb_resolve(members[i]));
        RBL_TRY(cancel_spec(members[i]));
        RBL_HIP(hipStreamSynchronize(members[i]->stream));
    }
    std::unique_ptr<rbl_group> g(new rbl_group());
    g->device = h0->cfg.device;
    RBL_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->shared_passes = h0->n > 0 && sweep_multi_supported(h0->storage, h0->ld);
    g->kpp = g->shared_passes ? sweep_multi_k(h0->storage, h0->ld) : 1;
    if (g->shared_passes) {
        const int rc = g->mem.alloc(&g->slab, sweep_multi_slab_doubles(h0->ld, h0->num_cu));
        if (rc != RBL_OK) {
            (void)hipStreamDestroy(g->stream);
            return rc;
        }
    }
    rbl_stats zero;
    std::memset(&zero, 0, sizeof(zero));
    for (int i = 0; i < k; ++i) {
        rbl_solver* h = members[i];
        g->m.push_back(h);
        g->live.push_back(1);
        g->saved_fused.push_back(h->fused_ok ? 1 : 0);
        g->saved_stream.push_back(h->stream);
        g->base_launches.push_back(h->nd_launches);
        g->last.push_back(zero);
        g->syncs.push_back(0);
        h->in_group = true;
        h->stream = g->stream;
        // two-pass structure for every member: whatever a single-sweep erm pass prepared ahead is dropped
        h->fused_ok = false;
        h->z_ready = h->p_valid = h->p_pending = h->pred_valid = false;
    }
    *out = g.release();
    return RBL_OK;
}

int rbl_group_destroy(rbl_group* g) {
    if (!g) return RBL_OK;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (size_t i = 0; i < g->m.size(); ++i) {
        rbl_solver* h = g->m[i];
        (void)zb_resolve(h);   // a verdict still pending was written on the group's stream
        if (h->stream == g->stream) h->stream = g->saved_stream[i];
        h->fused_ok = g->saved_fused[i] != 0;
        h->in_group = false;
    }
    if (g->stream) {
        (void)hipStreamSynchronize(g->stream);
        (void)hipStreamDestroy(g->stream);
    }
    delete g;   // g->mem frees the slab
    return RBL_OK;
}

int rbl_group_step(rbl_group* g, int want_objective, rbl_stats* out) {
    if (!g) {
        rbl_set_error("group handle is NULL");
        return RBL_ERR_INVALID;
    }
    RBL_HIP(hipSetDevice(g->device));
    const int K = (int)g->m.size();
    std::vector<int> idx;
    for (int i = 0; i < K; ++i)
        if (g->live[i]) idx.push_back(i);
    hipStream_t s = g->stream;
    for (int i : idx) g->syncs[i] = 0;
    // A + B: every member's own z-step
    for (int i : idx) {
        SyncBook book(g->syncs[i]);
        RBL_TRY(rbl_phase_m(g->m[i]));
        RBL_TRY(rbl_phase_z(g->m[i], nullptr));
    }
    // C: q_k = D^T c_k, D read once per kpp members
    if (g->shared_passes) {
        for (int i : idx) {
            rbl_solver* h = g->m[i];
            if (h->sorted_path && !h->zb.c_ready) RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, s));
            h->zb.c_ready = false;
            h->zb.q_done = h->zb.used;     // an unsettled z-step's q is redone with it, by the member alone (zb_resolve)
            h->s32.q_done = h->s32.used;
        }
        for (size_t b = 0; b < idx.size(); b += (size_t)g->kpp) {
            const int kk = (int)std::min(idx.size() - b, (size_t)g->kpp);
            const double* c[RBL_MULTI_KMAX];
            double* q[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                c[j] = g->m[idx[b + j]]->c;
                q[j] = g->m[idx[b + j]]->q;
            }
            rbl_solver* h0 = g->m[idx[b]];
            RBL_TRY(launch_sweep_q_multi(h0->storage, h0->D, h0->n, h0->ld, kk, c, g->slab, q, h0->num_cu, s));
            g->shared_q += 1;
        }
        for (int i : idx) {
            rbl_solver* h = g->m[i];
            h->pending_mask = 1;
            h->z_ready = false;
            if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[2], s));
        }
    } else {
        for (int i : idx) {
            SyncBook book(g->syncs[i]);
            RBL_TRY(rbl_phase_q(g->m[i]));
        }
    }
    // D: every member's own w-step (a z-step that was not certified is redone here, with its own q)
    for (int i : idx) {
        SyncBook book(g->syncs[i]);
        RBL_TRY(rbl_phase_w(g->m[i]));
    }
    // E: v_k = D w_k, lambda_k += rho_k (z_k - v_k), the primal residuals - D read once per kpp members
    if (g->shared_passes) {
        for (size_t b = 0; b < idx.size(); b += (size_t)g->kpp) {
            const int kk = (int)std::min(idx.size() - b, (size_t)g->kpp);
            const double *w[RBL_MULTI_KMAX], *z[RBL_MULTI_KMAX];
            double *lam[RBL_MULTI_KMAX], *v[RBL_MULTI_KMAX], *part[RBL_MULTI_KMAX], *red[RBL_MULTI_KMAX], rho[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                rbl_solver* h = g->m[idx[b + j]];
                w[j] = h->w;
                z[j] = h->z;
                lam[j] = h->lam;
                v[j] = h->v;
                part[j] = h->partials;
                red[j] = h->red;
                rho[j] = h->step_rho;
            }
            rbl_solver* h0 = g->m[idx[b]];
            RBL_TRY(launch_sweep_v_multi(h0->storage, h0->D, h0->n, h0->ld, kk, w, z, lam, v, rho, part, red, h0->num_cu, s));
            g->shared_v += 1;
        }
        for (int i : idx) {
            rbl_solver* h = g->m[i];
            h->fused_ran = false;
            h->fused_v_ran = true;
            h->v_valid = true;
            h->pending_mask = 2;
            h->want_obj = want_objective;
            h->obj_is_risk = false;
            if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], s));
            if (want_objective && h->sorted_path) {
                RBL_TRY(risk_from_v(h, h->v, h->red + 1));
                h->obj_is_risk = true;
            } else if (want_objective) {
                RBL_TRY(launch_loss_sum(h->cfg.loss, h->n, h->v, 1.0, h->partials, h->red + 1, s, h->rs));   // objective.py:11-24
            }
        }
    } else {
        for (int i : idx) {
            SyncBook book(g->syncs[i]);
            RBL_TRY(rbl_phase_dual(g->m[i], want_objective));
        }
    }
    // F: all statistics kernels first, ONE host wait (the last one's word: they complete in stream order), then the
    // stop tests and schedules
    for (int i : idx) RBL_TRY(phase_finish_part(g->m[i], nullptr, FIN_ENQUEUE));
    if (!idx.empty()) {
        rbl_solver* hl = g->m[idx.back()];
        SyncBook book(g->syncs[idx[0]]);
        rbl_spin_wait(reinterpret_cast<volatile int*>(hl->hstat + 15), 0, s);
    }
    for (int i : idx) {
        g_host_syncs = g->syncs[i];
        RBL_TRY(phase_finish_part(g->m[i], &g->last[i], FIN_DIGEST));
        if (g->last[i].converged) g->live[i] = 0;   // frozen where its own rbl_solve would have stopped
    }
    g_host_syncs = 0;
    if (out)
        for (int i = 0; i < K; ++i) out[i] = g->last[i];
    return RBL_OK;
}

int rbl_group_solve(rbl_group* g, int max_iter, int want_objective, rbl_stats* last, double* hist_objective,
                    double* hist_primal, double* hist_dual, double* hist_rho, int64_t* iters, int64_t cap) {
    if (!g) {
        rbl_set_error("group handle is NULL");
        return RBL_ERR_INVALID;
    }
    const int K = (int)g->m.size();
    if (max_iter <= 0)
        for (int i = 0; i < K; ++i) max_iter = std::max(max_iter, (int)g->m[i]->cfg.max_iter);
    std::vector<int64_t> done((size_t)K, 0);
    for (int it = 0; it < max_iter; ++it) {
        bool any = false;
        std::vector<char> was_live(g->live);
        for (int i = 0; i < K; ++i) any = any || was_live[i];
        if (!any) break;
        RBL_TRY(rbl_group_step(g, want_objective, nullptr));
        for (int i = 0; i < K; ++i) {
            if (!was_live[i]) continue;
            const rbl_stats& st = g->last[i];
            const int64_t k = done[i]++;
            if (k < cap) {
                if (hist_objective) hist_objective[i * cap + k] = st.objective;
                if (hist_primal) hist_primal[i * cap + k] = st.primal;
                if (hist_dual) hist_dual[i * cap + k] = st.dual;
                if (hist_rho) hist_rho[i * cap + k] = st.rho;
            }
        }
    }
    for (int i = 0; i < K; ++i) {
        if (iters) iters[i] = done[i];
        if (last) last[i] = g->last[i];
    }
    return RBL_OK;
}

int rbl_group_counters(rbl_group* g, int* k_per_pass, int64_t* shared_v, int64_t* shared_q, int64_t* single_passes) {
    if (!g) {
        rbl_set_error("group handle is NULL");
        return RBL_ERR_INVALID;
    }
    if (k_per_pass) *k_per_pass = g->kpp;
    if (shared_v) *shared_v = g->shared_v;
    if (shared_q) *shared_q = g->shared_q;
    if (single_passes)
        for (size_t i = 0; i < g->m.size(); ++i) single_passes[i] = g->m[i]->nd_launches - g->base_launches[i];
    return RBL_OK;
}

}  // extern "C"

// =================================================== kernel-level entry points (host buffers)
// They run on the same workspace allocators as the solver handle (alloc_sort, alloc_pav, alloc_prefix, alloc_wstep).
namespace {
struct Scratch {   // the buffers and the stream of one call
    DevArena mem;
    hipStream_t s = nullptr;
    ~Scratch() {
        if (s) (void)hipStreamDestroy(s);
    }
    template <typename T>
    int upload(T** p, const T* host, size_t count) {
        RBL_TRY(mem.alloc(p, count));
        if (count) RBL_HIP(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
        return RBL_OK;
    }
};

int scratch_begin(Scratch& sc, int* num_cu) {
    RBL_TRY(check_device(nullptr));
    RBL_HIP(hipStreamCreateWithFlags(&sc.s, hipStreamNonBlocking));
    if (num_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        RBL_HIP(hipGetDevice(&dev));
        RBL_HIP(hipGetDeviceProperties(&prop, dev));
        *num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return RBL_OK;
}

// D (host fp64 n x d) -> device storage with ld padding
int upload_matrix(Scratch& sc, int storage, int64_t n, int64_t d, const double* D, void** Dd, int64_t* ld_out) {
    const int64_t ld = round_up(d, 4);
    const size_t esz = storage == RBL_STORE_F32 ? 4 : 8;
    std::vector<unsigned char> host((size_t)n * ld * esz, 0);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t j = 0; j < d; ++j) {
            if (storage == RBL_STORE_F32) ((float*)host.data())[r * ld + j] = (float)D[r * d + j];
            else ((double*)host.data())[r * ld + j] = D[r * d + j];
        }
    RBL_TRY(sc.upload((unsigned char**)Dd, host.data(), host.size()));
    *ld_out = ld;
    return RBL_OK;
}
}  // namespace

extern "C" {

int rbl_k_prox(int loss, int64_t n, const double* sigma, double rho, const double* m, double* out) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0) return RBL_OK;
    double *ds = nullptr, *dm = nullptr, *dout = nullptr;
    RBL_TRY(sc.upload(&ds, sigma, (size_t)n));
    RBL_TRY(sc.upload(&dm, m, (size_t)n));
    RBL_TRY(sc.mem.alloc(&dout, (size_t)n));
    RBL_TRY(launch_prox(loss, n, ds, rho, dm, dout, sc.s));
    RBL_HIP(hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_sort(int64_t n, const double* keys, double* sorted_keys, uint32_t* perm) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0) return RBL_OK;
    double *dk = nullptr, *ms = nullptr;
    RBL_TRY(sc.upload(&dk, keys, (size_t)n));
    SortWorkspace sw{};
    RBL_TRY(alloc_sort(sc.mem, sw, n, true, sc.s));
    RBL_TRY(sc.mem.alloc(&ms, (size_t)n));
    RBL_TRY(launch_keys_from_m(n, dk, sw.keys[0], sw.vals[0], sc.s));
    RBL_TRY(launch_radix_sort(sw, n, true, sc.s));
    RBL_TRY(launch_unflip_keys(n, sw.keys[0], ms, sc.s));
    if (sorted_keys) RBL_HIP(hipMemcpyAsync(sorted_keys, ms, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    if (perm) RBL_HIP(hipMemcpyAsync(perm, sw.vals[0], sizeof(u32) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

// ncalls successive PAV solves on ONE workspace (m_sorted: ncalls x n): the hints of the upper seams, the barrier parity
// and the EHRM speculated branch carry over from one call to the next as they do between the z-steps of a solve.
static int k_pav_common(int loss, int64_t n, const double* sigma_a, const double* sigma_b, int ehrm, double B,
                        double rho, int ncalls, const double* m_sorted, int branch_in, int upper, double* out,
                        int64_t* n_merges, int* branch_out, uint32_t* counters_out) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0 || ncalls <= 0) return RBL_OK;
    double *sa = nullptr, *sb = nullptr;
    RBL_TRY(sc.upload(&sa, sigma_a, (size_t)n));
    if (ehrm) RBL_TRY(sc.upload(&sb, sigma_b, (size_t)n));
    else sb = sa;
    PavWorkspace pw{};   // the sorted m goes to pw.ms, its prefix sums to pw.pm
    RBL_TRY(alloc_pav(sc.mem, pw, n, sc.s));
    PrefixBufs pa, pb;
    RBL_TRY(alloc_prefix(sc.mem, pa, n));
    pb = pa;
    if (ehrm) RBL_TRY(alloc_prefix(sc.mem, pb, n));
    PavExtras ex = pw.ex;
    {
        int dev = 0, cus = 0;
        RBL_HIP(hipGetDevice(&dev));
        RBL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        ex.num_cu = cus;
    }
    ex.B = B;
    ex.upper = upper;
    {
        const char* e = getenv("RBL_EHRM_SPEC");   // 0 / 1: the speculated branch; -1: round 2's separate pass
        if (e && (atoi(e) == 0 || atoi(e) == 1)) ex.spec = atoi(e);
        // a forced branch (the tests pin both) and RBL_EHRM_SPEC=-1 go through the separate test; the automatic choice
        // through the speculation inside the bottom kernel
        if (!ehrm || branch_in >= 0 || (e && atoi(e) == -1)) ex.fpart = nullptr;
    }
    RBL_TRY(launch_prefix(sa, n, pa, sc.s));
    if (ehrm) RBL_TRY(launch_prefix(sb, n, pb, sc.s));
    // identity permutation scatter applies the EHRM clip
    std::vector<u32> idh((size_t)n);
    for (int64_t i = 0; i < n; ++i) idh[(size_t)i] = (u32)i;
    u32* idd = nullptr;
    double* zz = nullptr;
    RBL_TRY(sc.upload(&idd, idh.data(), (size_t)n));
    RBL_TRY(sc.mem.alloc(&zz, (size_t)n));
    for (int call = 0; call < ncalls; ++call) {
        RBL_HIP(hipMemcpyAsync(pw.ms, m_sorted + (size_t)call * n, sizeof(double) * n, hipMemcpyHostToDevice, sc.s));
        RBL_TRY(launch_prefix(pw.ms, n, pw.pm, sc.s));
        if (ehrm && !ex.fpart) RBL_TRY(launch_ehrm_branch(n, sa, sb, B, rho, pw.ms, pw.partials, pw.branch, branch_in, sc.s));
        RBL_TRY(launch_pav_tree(loss, n, rho, pw.ms, sa, sb, pw.u, pa.view(), pb.view(), pw.pm.view(), ehrm ? pw.branch : nullptr,
                                pw.recs, pw.counters, sc.s, nullptr, nullptr, &ex));
        RBL_TRY(launch_scatter_z(n, pw.u, idd, ehrm ? pw.branch : nullptr, B, ehrm, rho, nullptr, zz, nullptr, 0, n, sc.s));
        RBL_HIP(hipMemcpyAsync(out + (size_t)call * n, zz, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
        unsigned mc4[4] = {0, 0, 0, 0};
        int br = -1;
        RBL_HIP(hipMemcpyAsync(mc4, pw.counters, sizeof(mc4), hipMemcpyDeviceToHost, sc.s));
        if (ehrm) RBL_HIP(hipMemcpyAsync(&br, pw.branch, sizeof(int), hipMemcpyDeviceToHost, sc.s));
        RBL_HIP(hipStreamSynchronize(sc.s));
        if (counters_out)
            for (int j = 0; j < 4; ++j) counters_out[4 * call + j] = mc4[j];
        if (mc4[3] != 0) {
            rbl_set_error("PAV: the upper-level kernel did not complete (a wait gave up or its fill list overflowed)");
            return RBL_ERR_HIP;
        }
        if (n_merges) n_merges[call] = mc4[0];
        if (branch_out) branch_out[call] = br;
        if (ehrm && br >= 0) ex.spec = br;   // the next call speculates the branch this one took (rbl_phase_finish)
    }
    return RBL_OK;
}

int rbl_k_pav(int loss, int64_t n, const double* sigma, double rho, const double* m_sorted, double* out,
              int64_t* n_merges) {
    return k_pav_common(loss, n, sigma, sigma, 0, 0.0, rho, 1, m_sorted, -1, PAV_UPPER_DEFAULT, out, n_merges, nullptr,
                        nullptr);
}

int rbl_k_pav_ehrm(int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho,
                   const double* m_sorted, int branch, double* out, int* branch_out) {
    return k_pav_common(RBL_LOSS_BCE, n, sigma_a, sigma_b, 1, B, rho, 1, m_sorted, branch, PAV_UPPER_DEFAULT, out, nullptr,
                        branch_out, nullptr);
}

int rbl_k_pav_seq(int loss, int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho, int ncalls,
                  const double* m_sorted, int upper, double* out, int* branch_out, uint32_t* counters) {
    if (loss != RBL_LOSS_BCE && loss != RBL_LOSS_HINGE) {
        rbl_set_error("rbl_k_pav_seq: unknown loss %d", loss);
        return RBL_ERR_INVALID;
    }
    if (upper != RBL_PAV_UPPER_PERSIST && upper != RBL_PAV_UPPER_TWO_LAUNCH) {
        rbl_set_error("rbl_k_pav_seq: upper must be RBL_PAV_UPPER_PERSIST or RBL_PAV_UPPER_TWO_LAUNCH, got %d", upper);
        return RBL_ERR_INVALID;
    }
    const int ehrm = sigma_b != nullptr;
    if (ehrm && loss != RBL_LOSS_BCE) {
        rbl_set_error("rbl_k_pav_seq: the EHRM z-step is defined for the BCE loss only");
        return RBL_ERR_INVALID;
    }
    return k_pav_common(loss, n, sigma_a, ehrm ? sigma_b : sigma_a, ehrm, B, rho, ncalls, m_sorted, -1,
                        upper == RBL_PAV_UPPER_PERSIST ? PAV_UPPER_PERSIST : PAV_UPPER_TWO_LAUNCH, out, nullptr, branch_out,
                        counters);
}

int rbl_k_gemv(int storage, int64_t n, int64_t d, const double* D, const double* w, double* v) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    if (n <= 0) return RBL_OK;
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    std::vector<double> wp((size_t)ld, 0.0);
    for (int64_t j = 0; j < d; ++j) wp[(size_t)j] = w[j];
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(sc.upload(&dw, wp.data(), (size_t)ld));
    RBL_TRY(sc.mem.alloc(&dv, (size_t)n));
    RBL_TRY(launch_gemv(storage, Dd, n, ld, dw, dv, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(v, dv, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemvt(int storage, int64_t n, int64_t d, const double* D, const double* c, double* q) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n > 0 ? n : 0, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, c, (size_t)n));
    RBL_TRY(sc.mem.alloc(&slab, (size_t)gemvt_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_TRY(launch_gemvt(storage, Dd, n, ld, dc, slab, dq, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(q, dq, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemv_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* W, double* V) {
    if (k < 1 || k > 64 || d <= 0) {
        rbl_set_error("rbl_k_gemv_multi: 1..64 columns, d > 0");
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    if (n <= 0) return RBL_OK;
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    std::vector<double> wp((size_t)ld * k, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < d; ++i) wp[(size_t)j * ld + i] = W[(size_t)j * d + i];
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(sc.upload(&dw, wp.data(), wp.size()));
    RBL_TRY(sc.mem.alloc(&dv, (size_t)n * k));
    const bool multi = sweep_multi_supported(storage, ld);
    const int kpp = multi ? sweep_multi_k(storage, ld) : 1;
    for (int j0 = 0; j0 < k; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {   // outside the multi-column kernels' widths: the single-column pass per column
            RBL_TRY(launch_gemv(storage, Dd, n, ld, dw + (size_t)j0 * ld, dv + (size_t)j0 * n, num_cu, sc.s));
            continue;
        }
        const double* w[RBL_MULTI_KMAX];
        double* v[RBL_MULTI_KMAX];
        for (int j = 0; j < kk; ++j) {
            w[j] = dw + (size_t)(j0 + j) * ld;
            v[j] = dv + (size_t)(j0 + j) * n;
        }
        RBL_TRY(launch_sweep_v_multi(storage, Dd, n, ld, kk, w, nullptr, nullptr, v, nullptr, nullptr, nullptr, num_cu, sc.s));
    }
    RBL_HIP(hipMemcpyAsync(V, dv, sizeof(double) * n * k, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemvt_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* Cm, double* Q) {
    if (k < 1 || k > 64 || d <= 0) {
        rbl_set_error("rbl_k_gemvt_multi: 1..64 columns, d > 0");
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n > 0 ? n : 0, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, Cm, (size_t)(n > 0 ? n : 0) * k));
    const bool multi = n > 0 && sweep_multi_supported(storage, ld);
    const int kpp = multi ? sweep_multi_k(storage, ld) : 1;
    RBL_TRY(sc.mem.alloc(&slab, multi ? sweep_multi_slab_doubles(ld, num_cu) : (size_t)gemvt_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld * k));
    for (int j0 = 0; j0 < k; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {
            RBL_TRY(launch_gemvt(storage, Dd, n, ld, dc + (size_t)j0 * (n > 0 ? n : 0), slab, dq + (size_t)j0 * ld, num_cu, sc.s));
            continue;
        }
        const double* c[RBL_MULTI_KMAX];
        double* q[RBL_MULTI_KMAX];
        for (int j = 0; j < kk; ++j) {
            c[j] = dc + (size_t)(j0 + j) * n;
            q[j] = dq + (size_t)(j0 + j) * ld;
        }
        RBL_TRY(launch_sweep_q_multi(storage, Dd, n, ld, kk, c, slab, q, num_cu, sc.s));
    }
    for (int j = 0; j < k; ++j)
        RBL_HIP(hipMemcpyAsync(Q + (size_t)j * d, dq + (size_t)j * ld, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gram(int storage, int64_t n, int64_t d, const double* D, double* G) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *slab = nullptr, *dG = nullptr;
    RBL_TRY(sc.mem.alloc((unsigned char**)&slab, gram_slab_bytes(ld, num_cu, n > 0 ? n : 1)));
    RBL_TRY(sc.mem.alloc(&dG, (size_t)ld * ld));
    RBL_TRY(launch_gram(storage, Dd, n, ld, d, slab, dG, num_cu, sc.s));
    std::vector<double> hG((size_t)ld * ld);
    RBL_HIP(hipMemcpyAsync(hG.data(), dG, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int64_t i = 0; i < d; ++i)
        for (int64_t j = 0; j < d; ++j) G[i * d + j] = hG[(size_t)(i * ld + j)];
    return RBL_OK;
}

int rbl_k_wstep(int wstep, int64_t d, const double* G, const double* q, double rho, double reg, double smooth_t,
                const double* w0, double tol, double* w_out, int* iters) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    const int64_t ld = round_up(d, 4);
    std::vector<double> hG((size_t)ld * ld, 0.0), hq((size_t)ld, 0.0), hw((size_t)ld, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        for (int64_t j = 0; j < d; ++j) hG[(size_t)(i * ld + j)] = G[i * d + j];
        hq[(size_t)i] = q[i];
        hw[(size_t)i] = w0 ? w0[i] : 0.0;
    }
    double *dG = nullptr, *dq = nullptr, *dw = nullptr;
    RBL_TRY(sc.upload(&dG, hG.data(), hG.size()));
    RBL_TRY(sc.upload(&dq, hq.data(), hq.size()));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    double lam = 0.0;
    RBL_TRY(launch_power_iteration(dG, ld, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    int it = 0;
    RBL_TRY(run_wstep(wstep, dG, ld, dq, rho, reg, smooth_t, L, tol > 0.0 ? tol : 1e-13, 100000, dw, ww, &it, sc.s));
    RBL_HIP(hipMemcpyAsync(w_out, dw, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (iters) *iters = it;
    return RBL_OK;
}

int rbl_k_weights(int weight_function, int64_t n, const double* args, int n_args, double* alphas, double* betas) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (weight_function < RBL_W_ERM || weight_function > RBL_W_EHRM) {
        rbl_set_error("Unrecognized framework! Options: ['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']");
        return RBL_ERR_INVALID;
    }
    if (weight_function != RBL_W_ERM && weight_function != RBL_W_EHRM) {
        const int need = (weight_function == RBL_W_AORR || weight_function == RBL_W_AORR_DC) ? 2 : 1;
        if (!args || n_args < need) {
            rbl_set_error("args for framework is None!");
            return RBL_ERR_INVALID;
        }
    }
    double a2[2] = {args && n_args > 0 ? args[0] : 0.0, args && n_args > 1 ? args[1] : 0.0};
    double *da = nullptr, *db = nullptr;
    RBL_TRY(sc.mem.alloc(&da, (size_t)n));
    RBL_TRY(sc.mem.alloc(&db, (size_t)n));
    RBL_TRY(launch_weights(weight_function, n, a2, da, db, sc.s));
    if (alphas) RBL_HIP(hipMemcpyAsync(alphas, da, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    if (betas) RBL_HIP(hipMemcpyAsync(betas, db, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

}  // extern "C"
