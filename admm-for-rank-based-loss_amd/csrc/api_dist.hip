// api_dist.hip - the z-step of a row-sharded rank-weighted problem: the steps the driver runs between its collectives
// (rbl_zd_*: sample sort + chunked PAV with seam searches; rbl_zbd_*: the sort-free banded form).
#include "api_internal.h"

// ================================================================== distributed z-step
// Rank-weighted problems on several GPUs: the driver (dist.py: _z_distributed)
// calls these between its collectives; oracle/zdist.py restates every step on the CPU.
// Layout of RBL_BUF_ZD_SMALL (doubles): [0,256) samples | [256,259) bounds | [260,262) EHRM
// fvals | [320,384) candidates | [512, 512+3*4096) partial sums | [12800+..) seam sums.
namespace {
constexpr int ZD_OFF_SAMPLES = 0, ZD_OFF_BOUNDS = 256, ZD_OFF_FV = 260, ZD_OFF_CAND = 320, ZD_OFF_PART = 512,
              ZD_OFF_SUMS = 512 + 3 * 4096;
constexpr int ZD_MAX_CAND = 4096;   // world * K
}  // namespace

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

extern "C" {

int rbl_zd_sort_local(rbl_solver* h, int nsamples) {
    RBL_ENTER_ITER(h);
    RBL_TRY(zd_ensure(h));
    if (nsamples < 1 || nsamples > 256) {
        rbl_set_error("zd_sort_local: 1..256 samples");
        return RBL_ERR_INVALID;
    }
    hipStream_t s = h->stream;
    // keys of the local m, payload = GLOBAL row id
    if (!h->der.keys_ready) {
        RBL_TRY(launch_keys_from_m(h->n, h->m, h->sw.keys[0], h->sw.vals[0], s));
        if (h->off != 0) RBL_TRY(launch_add_u32(h->n, h->sw.vals[0], (u32)h->off, s));
    }
    h->der.keys_ready = false;
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
    h->der.keys_ready = false;
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
    if (!h->zb.enabled || !h->der.keys_ready) {
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
    if (!(h->zb.enabled && h->der.keys_ready && h->iter > 0 && h->iter >= h->zb.skip_until)) return RBL_OK;
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
    const int seq = h->zb.dv.arm();
    RBL_TRY(launch_zbd_decide(h->cfg.loss, h->zb.cfg, h->zb.st, k, h->step_rho, h->zb.tot, last, h->stream, h->zb.dv.pin, seq));
    RBL_TRY(h->zb.dv.wait(h->stream, "zbd_decide: the verdict of the root pass was never written"));
    *settled = h->zb.dv.word(1);
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
    const int seq = h->zb.v.arm();
    RBL_TRY(launch_zbd_apply(h->cfg.loss, h->zb.cfg, h->n, h->step_rho, h->m, h->z, h->lam, h->c, h->zb.st, h->zb.v.pin, seq,
                             h->pw.counters, h->stream));
    // every rank holds the same state, so every rank reads the same verdict and takes the same branch afterwards
    RBL_TRY(h->zb.v.wait(h->stream, "banded z-step: its status word was never written"));
    if (status) *status = h->zb.v.word(1);
    if (h->zb.v.word(1) == ZB_OK) {
        h->zb.backoff = 0;
        h->der.zb_c_ready = true;
        h->zb.mode = 1;
        h->der.keys_ready = false;
        if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[1], h->stream));
    } else {
        zb_back_off(h);   // mode 2: the caller runs the sort-based distributed z-step (rbl_zd_*) for this iteration
    }
    return RBL_OK;
}

}  // extern "C"
