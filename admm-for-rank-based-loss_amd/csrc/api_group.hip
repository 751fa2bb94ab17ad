// api_group.hip - groups: K problems on one D, one ADMM iteration of every live member per rbl_group_step with the two
// n x d passes shared (sweep_multi.hip; on RBL_STORE_CSR with RBL_GROUP_SHARE_SPARSE the multi-column passes of
// spmv.hip).  struct rbl_group: api_internal.h.
#include "api_internal.h"

extern "C" {

// The arena buffers of the shared sparse passes follow the store: the owner may have uploaded again since the last step
// (more rows cannot come, more segments can).  The new buffer first: a failed allocation leaves the group its old one.
static int group_sparse_room(rbl_group* g, const CsrStore* st) {
    const size_t want[2] = {(size_t)st->nseg * RBL_MULTI_KMAX, (size_t)st->n * RBL_MULTI_KMAX};
    double** buf[2] = {&g->slab, &g->cpack};
    size_t* have[2] = {&g->slab_doubles, &g->cpack_doubles};
    for (int i = 0; i < 2; ++i) {
        if (*buf[i] && want[i] <= *have[i]) continue;
        double* grown = nullptr;
        RBL_TRY(g->mem.alloc(&grown, want[i]));
        if (*buf[i]) {
            RBL_HIP(hipStreamSynchronize(g->stream));
            g->mem.release(*buf[i]);
        }
        *buf[i] = grown;
        *have[i] = want[i] > 0 ? want[i] : 1;
    }
    return RBL_OK;
}

int rbl_group_create(rbl_solver* const* members, int k, rbl_group** out) { return rbl_group_create_opts(members, k, 0, out); }

int rbl_group_create_opts(rbl_solver* const* members, int k, int flags, rbl_group** out) {
    if (!out) {
        rbl_set_error("group_create: out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = nullptr;
    if (flags & ~RBL_GROUP_SHARE_SPARSE) {
        rbl_set_error("group_create: unknown flag bits 0x%x (RBL_GROUP_SHARE_SPARSE is the only flag)", flags & ~RBL_GROUP_SHARE_SPARSE);
        return RBL_ERR_INVALID;
    }
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
        g->slab_doubles = sweep_multi_slab_doubles(h0->ld, h0->num_cu);
        const int rc = g->mem.alloc(&g->slab, g->slab_doubles);
        if (rc != RBL_OK) {
            (void)hipStreamDestroy(g->stream);
            return rc;
        }
    } else if ((flags & RBL_GROUP_SHARE_SPARSE) && h0->storage == RBL_STORE_CSR && h0->n > 0 && ((const CsrStore*)h0->D)->colptr) {
        // the opt-in: spmv.hip's multi-column passes, RBL_MULTI_KMAX members per read of the entries (on dense storage the
        // flag changes nothing: sweep_multi_supported alone decides there).  The buffers come with the first shared pass
        g->shared_passes = g->sparse = true;
        g->kpp = RBL_MULTI_KMAX;
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
        drop_look_ahead(h->der);
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
    for (hipEvent_t e : g->pev)
        if (e) (void)hipEventDestroy(e);
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
        for (int i : idx) RBL_TRY(q_prologue(g->m[i]));   // (an unsettled z-step's q is redone with it, by the member alone)
        const bool timed = g->profile && !idx.empty();
        if (timed) RBL_HIP(hipEventRecord(g->pev[0], s));
        for (size_t b = 0; b < idx.size(); b += (size_t)g->kpp) {
            const int kk = (int)std::min(idx.size() - b, (size_t)g->kpp);
            const double* c[RBL_MULTI_KMAX];
            double* q[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                c[j] = g->m[idx[b + j]]->c;
                q[j] = g->m[idx[b + j]]->q;
            }
            rbl_solver* h0 = g->m[idx[b]];
            if (g->sparse) {
                const CsrStore* st = (const CsrStore*)h0->D;
                RBL_TRY(group_sparse_room(g, st));
                RBL_TRY(launch_csr_gemvt_multi(st, h0->n, h0->ld, kk, c, g->cpack, g->cpack_doubles, g->slab, g->slab_doubles, q,
                                               h0->num_cu, s, timed && b == 0 && kk > 1 ? g->pev[2] : nullptr));
                if (b == 0) g->pack_timed = timed && kk > 1;
            } else {
                RBL_TRY(launch_sweep_q_multi(h0->storage, h0->D, h0->n, h0->ld, kk, c, g->slab, q, h0->num_cu, s));
            }
            g->shared_q += 1;
        }
        if (timed) RBL_HIP(hipEventRecord(g->pev[1], s));
        for (int i : idx) RBL_TRY(q_epilogue(g->m[i]));
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
    if (g->sparse) {
        // the sparse pass carries v alone: every member's dual update is rbl_phase_dual's unfused one behind it
        const bool timed = g->profile && !idx.empty();
        if (timed) RBL_HIP(hipEventRecord(g->pev[3], s));
        for (size_t b = 0; b < idx.size(); b += (size_t)g->kpp) {
            const int kk = (int)std::min(idx.size() - b, (size_t)g->kpp);
            const double* w[RBL_MULTI_KMAX];
            double* v[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                w[j] = g->m[idx[b + j]]->w;
                v[j] = g->m[idx[b + j]]->v;
            }
            rbl_solver* h0 = g->m[idx[b]];
            RBL_TRY(launch_csr_gemv_multi((const CsrStore*)h0->D, h0->n, kk, w, v, h0->num_cu, s));
            g->shared_v += 1;
        }
        if (timed) RBL_HIP(hipEventRecord(g->pev[4], s));
        for (int i : idx) {
            rbl_solver* h = g->m[i];
            h->fused_ran = h->fused_v_ran = false;
            RBL_TRY(dual_after_v(h, want_objective));
        }
    } else if (g->shared_passes) {
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
            h->fused_v_ran = h->der.v_valid = true;
            if (h->phase_timing) RBL_HIP(hipEventRecord(h->ev[4], s));
            RBL_TRY(dual_epilogue(h, want_objective, false));   // the pass carries no loss sum
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
        SyncBook book(g->syncs[idx[0]]);
        RBL_TRY(g->m[idx.back()]->fin.wait(s, FIN_NEVER));
    }
    for (int i : idx) {
        g_host_syncs = g->syncs[i];
        RBL_TRY(phase_finish_part(g->m[i], &g->last[i], FIN_DIGEST));
        if (g->last[i].converged) g->live[i] = 0;   // frozen where its own rbl_solve would have stopped
    }
    g_host_syncs = 0;
    if (g->profile && g->sparse && !idx.empty()) {   // the statistics are in: the events before them have completed
        float q = 0.f, v = 0.f, pk = 0.f;
        if (hipEventElapsedTime(&q, g->pev[0], g->pev[1]) == hipSuccess && hipEventElapsedTime(&v, g->pev[3], g->pev[4]) == hipSuccess &&
            (!g->pack_timed || hipEventElapsedTime(&pk, g->pev[0], g->pev[2]) == hipSuccess)) {
            g->pass_ms[0] += v;
            g->pass_ms[1] += q;
            g->pass_ms[2] += pk;
            g->pass_steps += 1;
        }
        (void)hipGetLastError();
    }
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

int rbl_group_profile(rbl_group* g, int on) {
    if (!g) {
        rbl_set_error("group handle is NULL");
        return RBL_ERR_INVALID;
    }
    RBL_HIP(hipSetDevice(g->device));
    if (on)
        for (hipEvent_t& e : g->pev)
            if (!e) RBL_HIP(hipEventCreate(&e));
    g->profile = on != 0;
    g->pass_ms[0] = g->pass_ms[1] = g->pass_ms[2] = 0.0;
    g->pass_steps = 0;
    return RBL_OK;
}

int rbl_group_pass_times(rbl_group* g, double* ms3, int64_t* steps) {
    if (!g || !ms3 || !steps) {
        rbl_set_error("group_pass_times: group, ms3 and steps must not be NULL");
        return RBL_ERR_INVALID;
    }
    for (int i = 0; i < 3; ++i) ms3[i] = g->pass_ms[i];
    *steps = g->pass_steps;
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
