// api_iter.hip - the ADMM iteration of src/optim/algorithms.py:119-164 as a sequence of device phases (rbl_phase_*,
// rbl_step, rbl_solve), the z-step on the sorted path with its back-offs (32-bit keys, sort-free banded z-step), and
// what evaluates an iterate: objective, accuracy, fairness statistics, risk.
#include "api_internal.h"

// Sparse storage keeps one partial sum per segment in the handle's own slab: it is regrown here when the data have more
// segments than it holds (a second upload on the owner of a borrowed D), and the launcher refuses a slab that is too small.
int ensure_sparse_slab(rbl_solver* h) {
    if (h->storage != RBL_STORE_CSR) return RBL_OK;
    const size_t need = sizeof(double) * (size_t)((const CsrStore*)h->D)->nseg;
    if (need > h->slab_bytes) {
        unsigned char* grown = nullptr;   // the new one first: a failed allocation leaves the handle its slab
        RBL_TRY(h->mem.alloc(&grown, need));
        RBL_HIP(hipStreamSynchronize(h->stream));
        h->mem.release(h->slab);
        h->slab = (double*)grown;
        h->slab_bytes = need;
    }
    return RBL_OK;
}

// q = D^T c of a handle
static int gemvt_h(rbl_solver* h, const double* c, double* q, hipEvent_t main_done = nullptr) {
    RBL_TRY(ensure_sparse_slab(h));
    return launch_gemvt(h->storage, h->D, h->n, h->ld, c, h->slab, q, h->num_cu, h->stream, main_done, h->slab_bytes / sizeof(double));
}

int op_data(rbl_solver* h, OpData* op) {
    RBL_TRY(ensure_sparse_slab(h));
    *op = OpData{(const CsrStore*)h->D, h->n, h->op_t, h->slab, h->slab_bytes / sizeof(double), h->op_part, h->num_cu};
    return RBL_OK;
}

int ensure_v(rbl_solver* h) {
    if (h->der.v_valid) return RBL_OK;
    h->nd_launches += 1;
    RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w, h->v, h->num_cu, h->stream));
    h->der.v_valid = true;
    return RBL_OK;
}

namespace {

// written by one thread behind the 32-bit sort's fix-up: its verdict for the host (sequence number last)
static __global__ void k_publish_flag(const int* __restrict__ flag, int* __restrict__ pin, int seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    pin[1] = flag[0];
    __threadfence_system();
    reinterpret_cast<volatile int*>(pin)[0] = seq;
}

// Sorted-path z-step over the n_total values in msrc (device), writing the local slice.
// allow32: the 32-bit-key sort may be used when rbl_phase_m prepared it (h->der.s32_m_ready) - its verdict is settled later
// (zb_resolve); false: 64-bit keys (the redo of an uncertified step, gathered m of the replicated distributed form).
int z_step_sorted(rbl_solver* h, const double* msrc, double rho, bool allow32 = true) {
    hipStream_t s = h->stream;
    const int64_t nt = h->nt;
    const u32* perm = h->sw.vals[0];
    const bool use32 = allow32 && h->der.s32_m_ready && msrc == h->m && nt == h->n;
    h->der.s32_m_ready = false;
    if (use32) {
        // fixed-point 32-bit keys of m: 4 radix passes over 8 bytes per row instead of 8 over 12, then one pass that gathers
        // the sorted m through the row ids and repairs the short runs the 32 bits cannot tell apart
        u32* k32 = reinterpret_cast<u32*>(h->sw.keys[0]);
        RBL_TRY(launch_keys32(nt, h->m, h->s32.mm, k32, h->sw.vals[0], (u32)h->off, s));
        RBL_TRY(launch_radix_sort32(h->sw, nt, s));
        RBL_TRY(launch_sort32_fix(nt, k32, h->sw.vals[0], h->m, (u32)h->off, h->pw.ms, h->sw.vals[1], h->s32.flag, s));
        const int seq = h->s32.v.arm();
        hipLaunchKernelGGL(k_publish_flag, dim3(1), dim3(64), 0, s, (const int*)h->s32.flag, h->s32.v.pin, seq);
        RBL_HIP(hipGetLastError());
        h->der.s32_used = true;
        h->der.s32_q_done = false;
        RBL_TRY(launch_prefix(h->pw.ms, nt, h->pw.pm, s));
        perm = h->sw.vals[1];
        h->sort_passes += 4;
    } else {
        // rbl_phase_m already formed the keys with m when it covers the whole problem (one pass instead of two)
        if (!(h->der.keys_ready && msrc == h->m && nt == h->n)) RBL_TRY(launch_keys_from_m(nt, msrc, h->sw.keys[0], h->sw.vals[0], s));
        RBL_TRY(launch_radix_sort(h->sw, nt, true, s));
        RBL_TRY(launch_unflip_prefix(h->sw.keys[0], nt, h->pw.ms, h->pw.pm, s));
        h->sort_passes += 8;
    }
    h->der.keys_ready = false;   // the sort consumes its input
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

}  // namespace

// Are the rank weights constant on a few bands (superquantile, aorr, aorr_dc)?  Then the z-step needs no sort
// (zband.hip).  Looked at once per handle, at the first rank-weighted z-step.
int zb_setup(rbl_solver* h) {
    h->zb.checked = true;
    h->zb.enabled = false;
    // RBL_NO_SORT32=1 (tests): rbl_phase_m never prepares the 32-bit keys, so every sorted z-step sorts 64-bit keys - the
    // run the default one is compared with bit for bit.  Looked at here, once per handle, like RBL_NO_ZBAND
    const char* no32 = getenv("RBL_NO_SORT32");
    h->s32.off = no32 && no32[0] == '1';
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
    RBL_TRY(h->mem.pinned(&h->zb.v.pin, 16, hipHostMallocDefault));
    for (int i = 0; i < 16; ++i) h->zb.v.pin[i] = 0;
    h->zb.dv.pin = h->zb.v.pin + 4;
    h->zb.enabled = true;   // set last: the buffers above are all there
    return RBL_OK;
}

// sum_i sigma_i * loss_(i) from n_total values of v (device) -> *out_dev
int risk_from_v(rbl_solver* h, const double* v_all, double* out_dev) {
    hipStream_t s = h->stream;
    if (h->cfg.weight_function == RBL_W_ERM) {
        h->risk_path = 1;
        return launch_loss_sum(h->cfg.loss, h->nt, v_all, 1.0 / (double)h->nt, h->partials, out_dev, s, h->rs, h->cw);
    }
    h->der.keys_ready = false;   // the sort workspace is reused: keys left by rbl_phase_m are gone
    RBL_TRY(launch_loss_keys(h->nt, v_all, h->sw.keys[0], s, h->rs));   // (own labels: the losses are taken at r * v)
    // piecewise-constant weights: the band sums of the losses need a select, not a sort (zband.hip; exact for any v)
    if (h->zb.enabled) {
        h->risk_path = 3;
        return launch_zband_risk(h->cfg.loss, h->zb.cfg, h->nt, h->sw.keys[0], h->zb.st, h->zb.hist, h->zb.part, out_dev, s);
    }
    h->risk_path = 2;
    RBL_TRY(launch_radix_sort(h->sw, h->nt, false, s));
    return launch_sorted_loss_dot(h->cfg.loss, h->nt, h->sw.keys[0], h->sigma_a, h->partials, out_dev, s);
}

// an uncertified sort-free z-step (here, and the sharded rbl_zbd_apply): the path pauses for 2, 4, ... 64 iterations
void zb_back_off(rbl_solver* h) {
    h->zb.backoff = h->zb.backoff < 2 ? 2 : (h->zb.backoff >= 32 ? 64 : 2 * h->zb.backoff);
    h->zb.skip_until = h->iter + 1 + h->zb.backoff;
    h->zb.mode = 2;
}

// The fast z-steps - the sort-free one (zband.hip) and the sort with 32-bit keys - report through pinned words
// (PinVerdict) whether they could certify their result.  Whoever is about to look at z (or at the q formed from it)
// before rbl_phase_w has done so settles it here: wait for the word; not certified -> the z-step (and q, if the q phase
// has run) is redone with the 64-bit sort + merge-tree PAV, and the fast path pauses (the sort-free one for 2, 4, ... 64
// iterations: the first iterations pool most of the rows in one block, that passes; 32-bit keys for 64).
// *redone (optional): tells rbl_phase_w that its w-step has to be repeated.
int zb_resolve(rbl_solver* h, bool* redone) {
    if (redone) *redone = false;
    bool q_done = false;
    if (h->der.s32_used) {
        // a run of equal keys too long for the fix-up (many m within range / 2^32 of each other: ties on a grid, a
        // degenerate range)
        h->der.s32_used = false;
        RBL_TRY(h->s32.v.settle(h->stream, "z-step: the verdict of the 32-bit sort was never written"));
        if (h->s32.v.word(1) == 0) return RBL_OK;
        h->s32.skip_until = h->iter + 1 + 64;
        q_done = h->der.s32_q_done;
        h->der.s32_q_done = false;
    } else if (h->der.zb_used) {
        h->der.zb_used = false;
        RBL_TRY(h->zb.v.settle(h->stream, "banded z-step: its status word was never written"));
        if (h->zb.v.word(1) == ZB_OK) {
            h->zb.backoff = 0;
            return RBL_OK;
        }
        zb_back_off(h);
        q_done = h->der.zb_q_done;
        h->der.zb_c_ready = h->der.zb_q_done = false;
    } else {
        return RBL_OK;
    }
    RBL_TRY(z_step_sorted(h, h->m, h->step_rho, false));
    if (q_done) {   // whichever pass formed it - the handle's own or a group's shared one - the redo is the handle's alone
        RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
        RBL_TRY(gemvt_h(h, h->c, h->q));
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
    if (h->wset) h->wset->w_replaced();
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

// L and the eigenbasis of G as rbl_gram_finish left them in the shared record: the owner behind its own rbl_gram_finish, a
// borrower whenever it catches up with the data epoch - it has no Gram calls of its own and takes the owner's word for G
void take_gram(rbl_solver* h) {
    const SharedData& r = *h->sd;
    h->L = r.L;
    h->ww.eig_Vt = r.eig_Vt;
    h->ww.eig_V = r.eig_V;
    h->ww.eig_lambda = r.eig_lambda;
    h->eig_sweeps = r.eig_sweeps;
    gram_finished(h->der, r.eig_ok);
}

// The owner has written a new D since this handle last looked: whatever the handle computed from the old D falls, a w-step
// enqueued ahead of time with it.  Run where a handle is about to iterate (require_ready) and by the evaluations that
// read D.  While a write has begun and not completed - it failed half way - the handle stays as it is: there is no D to
// compute anything from, and the call goes on to the refusals it met before (data_ready, the sparse launchers' guards).
int sync_data_epoch(rbl_solver* h) {
    if (h->epoch == h->sd->epoch || !h->sd->complete) return RBL_OK;
    RBL_TRY(cancel_spec(h));
    data_changed(h->der);
    h->epoch = h->sd->epoch;
    if (h->borrower) take_gram(h);
    return RBL_OK;
}

// ------------------------------------------------------------------------------- phases
int require_ready(rbl_solver* h) {
    if (h->cfg.objective_only) {
        rbl_set_error("objective-only handle cannot step");
        return RBL_ERR_STATE;
    }
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready) {
        rbl_set_error("step before set_data / generate_synthetic");
        return RBL_ERR_STATE;
    }
    if (!h->der.gram_ready) {
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

// What every form of the dual update ends with: the logged loss sum of an erm handle where the pass did not leave it, the
// flags of the exchange buffer, the rank-weighted risk.  own_loss_in_red: red[1] holds the handle's own loss sum already -
// the single-sweep pass' does (weights included; it never runs with own labels), k_dual's does unless the handle has own
// labels (k_dual sums the losses at v as the pass left it, the handle's own are at r * v) or row weights (k_dual sums
// unweighted losses); the V-only passes (launch_sweep_v, a group's launch_sweep_v_multi) leave none
int dual_epilogue(rbl_solver* h, int want_objective, bool own_loss_in_red) {
    if (!own_loss_in_red && want_objective && !h->sorted_path)
        RBL_TRY(launch_loss_sum(h->cfg.loss, h->n, h->v, 1.0, h->partials, h->red + 1, h->stream, h->rs, h->cw));   // objective.py:11-24
    h->pending_mask = 2 | (h->fused_ran ? 1 : 0);
    h->want_obj = want_objective;
    h->obj_is_risk = false;
    if (want_objective && h->sorted_path && h->nt == h->n) {
        RBL_TRY(risk_from_v(h, h->v, h->red + 1));
        h->obj_is_risk = true;
    }
    return RBL_OK;
}

// The unfused dual update behind a plain v = D w that is already in the stream - rbl_phase_dual's own launch_gemv, or a
// group's shared sparse pass (api_group.hip): lambda += rho (z - v) with the residual, then the epilogue.  The caller
// has cleared fused_ran / fused_v_ran.
int dual_after_v(rbl_solver* h, int want_objective) {
    h->der.v_valid = true;
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
    RBL_TRY(launch_dual(h->cfg.loss, h->n, h->step_rho, h->z, h->v, h->lam, h->partials, h->red, h->stream));
    return dual_epilogue(h, want_objective, !(h->rs || h->cw));
}

// Before q = D^T c in any form (the handle's own pass, a group's shared one).  Rank-weighted problems: the z-step's
// scatter writes z alone (one random access per row); c = z + lambda/rho (algorithms.py:192) is a streaming pass here.
// (Forming it inside the sweep was tried: the per-row division on the sweep's critical path costs 0.9 ms, the streaming
// pass 30 us.)  The q of an unsettled fast z-step is owed a redo with it (zb_resolve).
int q_prologue(rbl_solver* h) {
    if (h->sorted_path && !h->der.zb_c_ready) RBL_TRY(launch_make_c(h->n, h->z, h->lam, h->step_rho, h->c, h->stream));
    h->der.zb_c_ready = false;
    h->der.zb_q_done = h->der.zb_used;
    h->der.s32_q_done = h->der.s32_used;
    return RBL_OK;
}

int q_epilogue(rbl_solver* h, bool q_ahead) {
    h->pending_mask = q_ahead ? 0 : 1;  // a fused pass' q was already summed with its residuals
    h->der.z_ready = false;  // consumed: q (and zz) now belong to the iteration in flight
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[2], h->stream));
    return RBL_OK;
}

extern "C" {

int rbl_phase_m(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    RBL_TRY(require_ready(h));
    h->step_rho = h->rho;
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[0], h->stream));
    if (h->fused_ok && h->der.z_ready) return RBL_OK;
    RBL_TRY(ensure_v(h));
    if (h->sorted_path) {
        if (!h->zb.checked) RBL_TRY(zb_setup(h));
        // which z-step will follow on a single handle: the sort-free one (banded weights), else the sort - with 32-bit
        // keys from the second iteration on (iteration 0 starts from equal m: one run) unless a step was not certified
        const bool banded_next = h->zb.enabled && h->nt == h->n && h->iter > 0 && h->iter >= h->zb.skip_until;
        const bool s32 = h->s32.v.pin && !h->s32.off && h->nt == h->n && h->n >= 2 && h->iter > 0 &&
                         h->iter >= h->s32.skip_until && !banded_next;
        h->der.s32_m_ready = false;
        if (s32) {
            // m = D w - lambda/rho (algorithms.py:89) and its range (the 32-bit keys are a fixed-point image on it)
            RBL_TRY(launch_make_m_range(h->n, h->step_rho, h->v, h->lam, h->m, h->s32.mm, h->stream, h->rs));
            h->der.s32_m_ready = true;
            h->der.keys_ready = false;
        } else {
            // m and, in the same pass, the 64-bit sort's input for the z-step: keys of m with the GLOBAL row id as
            // payload (single GPU: off = 0; sharded: what rbl_zd_sort_local sorts)
            RBL_TRY(launch_make_m_keys(h->n, h->step_rho, h->v, h->lam, h->m, h->sw.keys[0], h->sw.vals[0], (u32)h->off,
                                       h->stream, h->rs));
            h->der.keys_ready = true;
        }
    }
    return RBL_OK;
}

int rbl_phase_z(rbl_solver* h, const void* m_all_dev) {
    RBL_ENTER_ITER(h);
    const double rho = h->step_rho;
    if (h->fused_ok && h->der.z_ready) {
        std::swap(h->z, h->z_next);  // the z-step of this iteration was done by the previous pass
    } else if (!h->sorted_path) {
        RBL_TRY(launch_erm_zc(h->cfg.loss, h->n, h->sigma0, rho, h->v, h->lam, h->m, h->z, h->c, h->stream, h->rs, h->sigw));
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
        if (h->zb.enabled && h->nt == h->n && h->der.keys_ready && msrc == h->m && h->iter > 0 && h->iter >= h->zb.skip_until) {
            const int seq = h->zb.v.arm();
            RBL_TRY(launch_zband(h->cfg.loss, h->zb.cfg, h->n, rho, h->sw.keys[0], h->m, h->z, h->lam, h->c, h->zb.st, h->zb.hist,
                                 h->zb.part, h->zb.v.pin, seq, h->pw.counters, h->stream, h->rs));
            h->der.zb_used = true;
            h->der.zb_q_done = false;
            h->der.zb_c_ready = true;   // the element-wise pass wrote c = z + lambda/rho as well
            h->zb.mode = 1;
        } else {
            h->der.zb_c_ready = false;
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
    z_replaced(h->der);   // with whatever the library's own z-step left behind: c, a verdict still unread
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
    RBL_TRY(launch_w_stats(h->ld, h->w, h->w_prev, h->red2, h->stream, h->ww.pen_l1, h->ww.pen_l2,
                           pen_terms(h)));   // dual residual, regulariser terms
    // no rho prediction was made for this w: the dual update runs unfused, and the d-space recurrence for
    // D^T lambda is re-seeded by the next rbl_phase_q (a caller that skipped rbl_phase_q: nothing of a previous pass is
    // pending any more)
    w_changed(h->der);
    if (h->wset) h->wset->w_replaced();
    drop_look_ahead(h->der);
    h->inner_iters = 0;
    h->ww.form = -1;
    if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[3], h->stream));
    return RBL_OK;
}

int rbl_phase_q(rbl_solver* h) {
    RBL_ENTER_ITER(h);
    const bool q_ahead = h->fused_ok && h->der.z_ready;
    if (!q_ahead) {
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[2], h->stream));
        RBL_TRY(q_prologue(h));
        RBL_TRY(gemvt_h(h, h->c, h->q, prof_now(h) ? h->kev[3] : nullptr));
        h->nd_launches += 1;
        if (prof_now(h)) h->kev_pending[1] = h->n > 0;
        if (h->fused_ok && !h->der.p_valid) {
            // D^T lambda seeds the d-space recurrence used to predict the primal residual
            RBL_TRY(gemvt_h(h, h->lam, q_pinit(h)));
            h->nd_launches += 1;
            h->der.p_pending = true;
        }
    }
    return q_epilogue(h, q_ahead);
}

// the single-sweep iteration's statistics kernel (launch_predict_rho) knows the two norms only: the weighted sums
// come from a launch of their own behind it
static int pen_terms_after_predict(rbl_solver* h) {
    if (!h->pen) return RBL_OK;
    return launch_pen_terms(h->ld, h->w, h->ww.pen_l1, h->ww.pen_l2, pen_terms(h), h->stream);
}

static int phase_w_body(rbl_solver* h) {
    const bool spec = h->spec_w;   // this w-step (and what follows it) was enqueued by the previous rbl_phase_finish
    h->spec_w = false;
    int wstep = h->cfg.wstep;
    if (!spec && (wstep != RBL_WSTEP_L1 || h->no_gram))   // the lasso kernel saves its warm start itself
        RBL_HIP(hipMemcpyAsync(h->w_prev, h->w, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
    if (h->der.p_pending) {
        RBL_HIP(hipMemcpyAsync(h->p, q_pinit(h), sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
        h->der.p_pending = false;
        h->der.p_valid = true;
    }
    // The lasso's active-set kernel reports its status through pinned memory; the statistics of
    // the new w and the rho prediction are enqueued behind it before the host looks at the
    // status, so the device works through them while the host waits.  Only when the kernel did
    // not converge (FISTA then changes w again) are they enqueued a second time.
    bool fs_pending = spec;
    const bool predict = h->fused_ok && h->der.p_valid;
    // the active-set lasso kernel leaves G w of its solution in ww.Gy (it needs the gradient for its
    // own optimality test): no d x d product for the rho prediction unless FISTA had to take over
    bool gw_ready = predict && wstep == RBL_WSTEP_L1;
    if (!spec && h->no_gram) {
        // no G: CG / FISTA on the operator rho D^T D + diag(.) (wstep_op.hip); csr never runs the single-sweep pass, so
        // there is no rho prediction and the statistics of the new w follow as on the !predict branch
        OpData op;
        RBL_TRY(op_data(h, &op));
        if (h->wset && wstep == RBL_WSTEP_L1) {
            // the exact working-set lasso (wstep_ws.hip); Gs belongs to the data epoch it was formed in
            if (h->wset->epoch != h->sd->epoch) {
                h->wset->built = false;
                h->wset->epoch = h->sd->epoch;
            }
            RBL_TRY(run_wstep_ws(op, h->ld, h->d, h->q, h->step_rho, h->cfg.reg, h->L, h->cfg.w_tol, 100000, h->w, h->ww, *h->wset,
                                 WS_CAP, h->pen ? h->pen_host.data() : nullptr, &h->inner_iters, h->stream));
        } else {
            RBL_TRY(run_wstep_op(wstep, op, h->ld, h->q, h->step_rho, h->cfg.reg, h->L, h->cfg.w_tol, 100000, h->w, h->ww,
                                 &h->inner_iters, h->stream));
        }
        fs_pending = false;
    } else if (!spec) {
        h->ww.eig_ok = h->der.eig_ok;   // (run_wstep's view of it)
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
            RBL_TRY(pen_terms_after_predict(h));
        } else {
            RBL_TRY(launch_w_stats(h->ld, h->w, h->w_prev, h->red2, h->stream, h->ww.pen_l1, h->ww.pen_l2, pen_terms(h)));
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
    h->der.pred_valid = false;
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
        h->der.pred_valid = true;
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
    // the first pass may have changed S for the w it produced (a cold start, an eviction): w_prev's support is found again
    if (h->wset) h->wset->w_replaced();
    return phase_w_body(h);
}

int rbl_phase_dual(rbl_solver* h, int want_objective) {
    RBL_ENTER_ITER(h);

    h->fused_ran = false;
    h->fused_v_ran = false;
    h->nd_launches += 1;
    if (h->fused_ok && h->der.pred_valid) {
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[4], h->stream));
        RBL_TRY(launch_sweep_erm(h->storage, h->cfg.loss, h->D, h->n, h->ld, h->w, h->z, h->lam, h->v, h->z_next,
                                 h->sigma0, h->step_rho, h->pred, h->slab, h->partials, h->q, h->red, q_zz(h),
                                 h->num_cu, h->stream, prof_now(h) ? h->kev[5] : nullptr, want_objective, nullptr, h->sigw,
                                 h->cw));
        if (prof_now(h)) h->kev_pending[2] = h->n > 0;
        h->fused_ran = true;
        h->der.v_valid = want_objective != 0;   // without objective logging the pass does not store v (ensure_v recomputes it if a misprediction asks)
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
        return dual_epilogue(h, want_objective, true);
    }
    if (h->fuse_v) {
        // v = D w and the lambda update in one pass (timed as the gemv of the iteration)
        if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[0], h->stream));
        RBL_TRY(launch_sweep_v(h->storage, h->D, h->n, h->ld, h->w, h->z, h->lam, h->v, h->step_rho, h->partials, h->red,
                               h->num_cu, h->stream, prof_now(h) ? h->kev[1] : nullptr));
        if (prof_now(h)) h->kev_pending[0] = h->n > 0;
        h->der.v_valid = true;
        h->fused_v_ran = true;
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], h->stream));
        return dual_epilogue(h, want_objective, false);
    }
    if (prof_now(h)) RBL_HIP(hipEventRecord(h->kev[0], h->stream));
    RBL_TRY(launch_gemv(h->storage, h->D, h->n, h->ld, h->w, h->v, h->num_cu, h->stream));
    if (prof_now(h)) {
        RBL_HIP(hipEventRecord(h->kev[1], h->stream));
        h->kev_pending[0] = true;
    }
    return dual_after_v(h, want_objective);
}

// One thread gathers the iteration's scalars into the pinned host block: the host then needs a
// single stream wait and no copies (each small device-to-host copy costs ~15 us of stream time).
static __global__ void k_pack_stats(const double* __restrict__ red, const double* __restrict__ red2,
                             const double* __restrict__ pred, const int* __restrict__ branch,
                             const unsigned* __restrict__ counters, int* __restrict__ zd_err,
                             double* __restrict__ hstat, int seq, const double* __restrict__ pen4) {
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
    hstat[11] = pen4 ? pen4[2] : 0.0;   // per-coordinate penalties: sum l1_j |w_j|, sum l2_j w_j^2
    hstat[12] = pen4 ? pen4[3] : 0.0;
    __threadfence_system();
    reinterpret_cast<volatile int*>(hstat + 15)[0] = seq;   // written last: the host polls this word
}

int rbl_phase_finish(rbl_solver* h, rbl_stats* out) {
    RBL_ENTER_ITER(h);
    return phase_finish_part(h, out, FIN_ALL);
}

}  // extern "C"

int phase_finish_part(rbl_solver* h, rbl_stats* out, int part) {
    float spec_ms = 0.f;   // the w-step of THIS iteration ran before its ev[0]: add its time back
    if (h->spec_timed) (void)hipEventElapsedTime(&spec_ms, h->ev_spec[0], h->ev_spec[1]);
    h->spec_timed = false;
    if (h->phase_timing && part != FIN_DIGEST) RBL_HIP(hipEventRecord(h->ev[5], h->stream));
    if (part != FIN_DIGEST) {
        const int pack_seq = h->fin.arm();
        hipLaunchKernelGGL(k_pack_stats, dim3(1), dim3(64), 0, h->stream, h->red, h->red2,
                           h->fused_ran ? h->pred : (const double*)nullptr,
                           (h->sorted_path && h->cfg.weight_function == RBL_W_EHRM) ? h->pw.branch : (const int*)nullptr,
                           h->sorted_path ? h->pw.counters : (const unsigned*)nullptr, h->zd_err, h->hstat, pack_seq,
                           (const double*)pen_terms(h));
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
    const bool try_spec = part == FIN_ALL && h->fused_ran && h->der.p_valid && h->cfg.wstep == RBL_WSTEP_L1 && !no_spec;
    if (try_spec) {
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev_spec[0], h->stream));
        bool fs_pending = false;
        RBL_TRY(run_wstep(RBL_WSTEP_L1, h->G, h->ld, h->q, 1.0, h->cfg.reg, h->smooth_t, h->L, h->cfg.w_tol, 100000, h->w,
                          h->ww, nullptr, h->stream, &fs_pending, h->pred, h->w_prev, true));   // leaves G w in ww.Gy
        RBL_TRY(launch_predict_rho(h->ld, h->q, h->p, h->p_alt, h->w, h->w_prev, h->ww.Gy, q_zz(h), 0.0,
                                   217.0 * (double)h->d, h->pred, h->red2, h->stream, h->pred));
        RBL_TRY(pen_terms_after_predict(h));
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev_spec[1], h->stream));
    }
    RBL_TRY(part == FIN_ALL ? h->fin.wait(h->stream, FIN_NEVER) : h->fin.check(FIN_NEVER));   // FIN_DIGEST: the group has waited
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
        if (h->pen) objective += 0.5 * (hs[11] + hs[12]);                           // R(w) = 1/2 sum (l1_j |w_j| + l2_j w_j^2)
        else if (h->cfg.wstep == RBL_WSTEP_L2) objective += 0.5 * h->cfg.reg * r2[1];   // objective.py:83-84
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
        h->der.z_ready = !conv && pr[0] == rho_next;
        if (!conv && !h->der.z_ready) mispred = 1;
        h->n_fused += 1;
        h->n_mispred += mispred;
    }
    h->der.pred_valid = false;
    if (try_spec) {
        if (!conv && h->der.z_ready) {
            h->spec_w = true;
            h->spec_timed = h->phase_timing;
        } else {
            RBL_HIP(hipMemcpyAsync(h->w, h->w_prev, sizeof(double) * h->ld, hipMemcpyDeviceToDevice, h->stream));
            if (h->wset) h->wset->w_replaced();
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

extern "C" {

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
    w_changed(h->der);
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

// w (host, d values) -> w_tmp on the device, m = D w_tmp: the scores the evaluations below start from
static int predict_into_m(rbl_solver* h, const double* w) {
    RBL_HIP(hipMemcpyAsync(h->w_tmp, w, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
    return launch_gemv(h->storage, h->D, h->n, h->ld, h->w_tmp, h->m, h->num_cu, h->stream);
}

int rbl_objective(rbl_solver* h, const double* w, int include_reg, double* out) {
    RBL_ENTER(h);
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready || !w || !out) {
        rbl_set_error("objective: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    if (h->nt != h->n) {
        rbl_set_error("objective: sharded handle - use the phase API");
        return RBL_ERR_STATE;
    }
    RBL_TRY(predict_into_m(h, w));
    RBL_TRY(risk_from_v(h, h->m, h->red2 + 4));
    double pr4[4] = {0.0, 0.0, 0.0, 0.0};
    if (h->pen) {
        RBL_TRY(launch_pen_terms(h->ld, h->w_tmp, h->ww.pen_l1, h->ww.pen_l2, h->pen + 2 * h->ld + 4, h->stream));
        RBL_HIP(hipMemcpyAsync(pr4, h->pen + 2 * h->ld + 4, sizeof(double) * 4, hipMemcpyDeviceToHost, h->stream));
    } else {
        RBL_TRY(launch_reg_terms(h->ld, h->w_tmp, h->red2 + 5, h->stream));
    }
    double r[3];
    RBL_HIP(hipMemcpyAsync(r, h->red2 + 4, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    double val = r[0];
    if (include_reg && h->pen) {
        val += 0.5 * (pr4[2] + pr4[3]);
    } else if (include_reg && h->cfg.reg > 0.0) {
        if (h->cfg.wstep == RBL_WSTEP_L2) val += 0.5 * h->cfg.reg * r[1];
        else val += 0.5 * h->cfg.reg * r[2];
    }
    *out = val;
    return RBL_OK;
}

// fraction of correctly classified rows of this handle's data (src/util/calculate_acc.py:3-19)
int rbl_accuracy(rbl_solver* h, const double* w, double threshold, double* out) {
    RBL_ENTER(h);
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready || !w || !out) {
        rbl_set_error("accuracy: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    if (!(threshold > 0.0 && threshold < 1.0)) {
        rbl_set_error("accuracy: threshold must be in (0, 1)");
        return RBL_ERR_INVALID;
    }
    RBL_TRY(predict_into_m(h, w));
    RBL_TRY(launch_accuracy(h->cfg.loss, h->n, h->m, h->ysign, std::log(threshold / (1.0 - threshold)), h->partials,
                            h->red2 + 4, h->stream, h->rs));
    double cnt = 0.0;
    RBL_HIP(hipMemcpyAsync(&cnt, h->red2 + 4, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    *out = h->n > 0 ? cnt / (double)h->n : 0.0;   // local rows; sharded callers average by n
    return RBL_OK;
}

// why the last sort-free z-step was (not) certified: the pinned status word stays as written until the next one is launched
int rbl_zband_status(rbl_solver* h, int* status, int* split) {
    RBL_ENTER(h);
    const bool have = h->zb.v.pin && h->zb.v.seq > 0 && h->zb.v.there();
    if (status) *status = have ? h->zb.v.word(1) : -1;
    if (split) *split = have ? h->zb.v.word(2) : -1;
    return RBL_OK;
}

// which kernels the handle's last risk went through (risk_from_v records it; read-only)
int rbl_risk_path(rbl_solver* h, int* path) {
    if (!h || !path) {
        rbl_set_error("risk_path: NULL argument");
        return RBL_ERR_INVALID;
    }
    *path = h->risk_path;
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

// SPD, DI, EOD, AOD, TI, FNRD of the linear classifier on this handle's rows
// (src/util/fair_metric.py:3-41); group: n doubles with values 0 / 1
int rbl_fair_statistics(rbl_solver* h, const double* w, const double* group, double threshold, double* out6) {
    RBL_ENTER(h);
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready || !w || !group || !out6) {
        rbl_set_error("fair_statistics: no data or NULL argument");
        return RBL_ERR_STATE;
    }
    double c[14];
    {
        DevArena mem;   // the group vector, freed after the readback
        double* gd = nullptr;
        RBL_TRY(mem.alloc(&gd, (size_t)h->n));
        if (hipMemcpyAsync(gd, group, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rbl_set_error("fair_statistics: upload failed");
            return RBL_ERR_HIP;
        }
        RBL_TRY(predict_into_m(h, w));
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

}  // extern "C"
