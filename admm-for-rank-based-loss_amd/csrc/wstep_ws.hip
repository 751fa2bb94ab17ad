// wstep_ws.hip - the exact working-set lasso / elastic net of a handle without a Gram matrix (RBL_CREATE_WORKING_SET on
// RBL_CREATE_NO_GRAM, storage RBL_STORE_CSR), fp64.  The w-step
//     min 1/2 w'(D^T D + diag(l2)/rho) w - q'w + sum_j kappa_j |w_j|,   kappa_j = l1_j / (2 rho) or reg / (2 rho)
// (reference: src/optim/algorithms.py:190-202, src/util/fast_lasso.py) is solved on a working set S of at most WS_CAP
// columns whose sub-Gram matrix Gs = D_S^T D_S is formed from the entries and kept across w-steps (it depends on D alone):
//   1. solve: gather q_S, w_S (l1_S, l2_S), run the Gram route's l1 w-step on (Gs, q_S) unchanged - the active-set kernel
//      of lasso_fs.hip, FISTA on Gs behind it when the active set outgrows it - and scatter w_S back.  No sparse pass.
//      Unused slots are inert: zero row and column of Gs, q = 0, so g = 0 exactly.
//   2. scan: g = D^T (D w) + (l2/rho) .* w - q through the two sparse passes (w = 0: g = -q, no pass).  Column j outside S
//      is a CANDIDATE when |g_j| - kappa_j > tol * max(1, max_j |q_j|), tol the w-step's own tolerance.  Per chunk of
//      OP_CHUNK columns (wstep_op_plan.h) the largest violation is taken, ties to the smaller index; one block then takes
//      up to WS_SELECT chunk winners, largest first, ties to the smaller index.  A function of ld alone: no grid enters.
//      No candidate: done - the KKT conditions hold on all columns.
//   3. grow: the chosen columns are appended to S (slots with w = 0 that are not free coordinates are evicted first when
//      S is full, Gs compacted), k_ws_gram_rows forms their rows and columns of Gs, back to 1.
// Invariant: every j with w_j != 0 is in S; everything outside S is +0.0, padding included.  Where S cannot hold what it
// must (or the rounds run out) the w-step leaves the route: run_wstep_op's FISTA from the current w, form 4.
//
// Gs[a][b] = one fma chain from +0.0 over the entries of column S[a] in ascending row, adding x_rj * x_ri where the row has
// an entry in column i = S[b].  The same products arrive in the same order from either side: Gs is symmetric in bits
// whichever column came first, and the grid enters no bit.  No atomics.
#include "rbl_internal.h"
#include "device_math.h"
#include "wstep_op_plan.h"

namespace {

constexpr int WG_THREADS = 256;
constexpr int WG_WPB = WG_THREADS / RBL_WAVE;   // 4 waves, WS_CAP doubles of LDS each: 32 KB

// the wave's LDS operations are issued in order; this keeps the compiler from moving them across a step in which
// another lane of the wave touches the same accumulator slot (spgram.hip: sg_wave_order)
// a value every lane holds alike, moved to scalar registers: the loops it bounds are uniform to the compiler as well
__device__ inline long long ws_uniform(long long v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL)), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}

__device__ inline void ws_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One wave per new slot m_old + item (column j = S[slot]).  The wave walks column j's entries in order, 64 (row, x_rj,
// row range) at a time in its lanes; per row the lanes stride over the row's entries and add x_rj * x_rc to acc[pos[c]]
// for the columns c in S.  Columns are distinct within a row and the wave's LDS operations are in order: no atomic, no
// barrier.  While row i is accumulated the first 64 entries of row i + 1 are in flight.  Then row `slot` of Gs is
// written whole (slots beyond the working set get the +0.0 they hold) and the mirror column for the slots < m_old; the
// new x new block is covered by the rows.
__global__ __launch_bounds__(WG_THREADS) void k_ws_gram_rows(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                             const double* __restrict__ val, const int64_t* __restrict__ colptr,
                                                             const int* __restrict__ row, const double* __restrict__ cval,
                                                             const int* __restrict__ pos, const int* __restrict__ S, int m_old,
                                                             int nnew, double* __restrict__ Gs) {
    extern __shared__ double ws_lds[];
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / RBL_WAVE);
    double* acc = ws_lds + (size_t)wave * WS_CAP;
    for (int item = (int)blockIdx.x * WG_WPB + wave; item < nnew; item += (int)gridDim.x * WG_WPB) {
        const int slot = m_old + item;
        const int j = S[slot];
        const long long begin = colptr[j], end = colptr[j + 1];
        for (int i = lane; i < WS_CAP; i += RBL_WAVE) acc[i] = 0.0;
        ws_wave_order();
        for (long long k0 = begin; k0 < end; k0 += RBL_WAVE) {
            const int cnt = (int)(end - k0 < RBL_WAVE ? end - k0 : RBL_WAVE);
            long long a = 0, e = 0;
            double x = 0.0;
            if (lane < cnt) {
                const int r = row[k0 + lane];
                x = cval[k0 + lane];
                a = indptr[r];
                e = indptr[r + 1];
            }
            long long ra = ws_uniform(__shfl(a, 0, RBL_WAVE)), re = ws_uniform(__shfl(e, 0, RBL_WAVE));
            int p = -1;
            double v = 0.0;
            if (ra + lane < re) {
                p = pos[col[ra + lane]];
                v = val[ra + lane];
            }
            for (int i = 0; i < cnt; ++i) {
                const double xr = __shfl(x, i, RBL_WAVE);
                const long long ca = ra, ce = re;
                const int pp = p;
                const double cv = v;
                if (i + 1 < cnt) {
                    ra = ws_uniform(__shfl(a, i + 1, RBL_WAVE));
                    re = ws_uniform(__shfl(e, i + 1, RBL_WAVE));
                    p = -1;
                    v = 0.0;
                    if (ra + lane < re) {
                        p = pos[col[ra + lane]];
                        v = val[ra + lane];
                    }
                }
                if (pp >= 0) acc[pp] = fma(xr, cv, acc[pp]);
                // a row of more than 64 entries: the rest (ca, ce are the wave's: a uniform loop)
                for (long long t = ca + RBL_WAVE; t < ce; t += RBL_WAVE) {
                    int p2 = -1;
                    double v2 = 0.0;
                    if (t + lane < ce) {
                        p2 = pos[col[t + lane]];
                        v2 = val[t + lane];
                    }
                    if (p2 >= 0) acc[p2] = fma(xr, v2, acc[p2]);
                }
                ws_wave_order();
            }
        }
        double* out = Gs + (size_t)slot * WS_CAP;
        for (int i = lane; i < WS_CAP; i += RBL_WAVE) out[i] = acc[i];
        for (int i = lane; i < m_old; i += RBL_WAVE) Gs[(size_t)i * WS_CAP + slot] = acc[i];
        ws_wave_order();
    }
}

struct WsCols {
    int n;
    int col[WS_SELECT];
};

// S[m_old + i] = col[i], pos[col[i]] = m_old + i
__global__ void k_ws_append(WsCols c, int m_old, int* __restrict__ S, int* __restrict__ pos) {
    const int i = (int)threadIdx.x;
    if (blockIdx.x == 0 && i < c.n) {
        S[m_old + i] = c.col[i];
        pos[c.col[i]] = m_old + i;
    }
}

// pos[S[a]] = val ? a : -1 for a < m (before / after an eviction rewrites S)
__global__ void k_ws_setpos(const int* __restrict__ S, int m, int set, int* __restrict__ pos) {
    const int a = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (a < m) pos[S[a]] = set ? a : -1;
}

// slot <- column: q_S, w_S and, with penalties, l1_S, l2_S; the unused slots get +0.0
__global__ void k_ws_gather(const int* __restrict__ S, int m, const double* __restrict__ q, const double* __restrict__ w,
                            const double* __restrict__ l1, const double* __restrict__ l2, double* __restrict__ qS,
                            double* __restrict__ wS, double* __restrict__ l1S, double* __restrict__ l2S) {
    const int a = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (a >= WS_CAP) return;
    const bool in = a < m;
    const int j = in ? S[a] : 0;
    qS[a] = in ? q[j] : 0.0;
    wS[a] = in ? w[j] : 0.0;
    if (l1) {
        l1S[a] = in ? l1[j] : 0.0;
        l2S[a] = in ? l2[j] : 0.0;
    }
}

// column <- slot; info[0] = coefficients != 0 (one block)
__global__ __launch_bounds__(WG_THREADS) void k_ws_scatter(const int* __restrict__ S, int m, const double* __restrict__ wS,
                                                           double* __restrict__ w, int* __restrict__ info) {
    __shared__ int nz;
    if (threadIdx.x == 0) nz = 0;
    __syncthreads();
    int mine = 0;
    for (int a = (int)threadIdx.x; a < m; a += WG_THREADS) {
        const double x = wS[a] == 0.0 ? 0.0 : wS[a];   // (a -0.0 of the solve becomes +0.0: everything outside the support is +0.0 in bits)
        w[S[a]] = x;
        mine += x != 0.0;
    }
    if (mine) atomicAdd(&nz, mine);
    __syncthreads();
    if (threadIdx.x == 0) info[0] = nz;
}

// out[a][b] = in[keep[a]][keep[b]] for a, b < m_new, +0.0 elsewhere (out != in)
__global__ void k_ws_compact(const double* __restrict__ in, double* __restrict__ out, const int* __restrict__ keep, int m_new) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)WS_CAP * WS_CAP) return;
    const int a = (int)(idx / WS_CAP), b = (int)(idx % WS_CAP);
    out[idx] = (a < m_new && b < m_new) ? in[(size_t)keep[a] * WS_CAP + keep[b]] : 0.0;
}

// (value, index) maximum: the larger value, ties to the smaller index - a total order, so the fold's shape enters no bit
__device__ inline void ws_better(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
__device__ inline void ws_block_argmax(double& v, int& idx, double* sv, int* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        ws_better(v, idx, ov, oi);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = v;
        si[threadIdx.x >> 6] = idx;
    }
    __syncthreads();
    v = sv[0];
    idx = si[0];
    for (int k = 1; k < OP_THREADS / 64; ++k) ws_better(v, idx, sv[k], si[k]);
    __syncthreads();
}

constexpr double WS_NONE = -1.0e300;   // "no column outside S in this chunk"

// The scan over the chunks of wstep_op_plan.h.  g_j = Gy_j + (l2_j / rho) w_j - q_j (Gy == NULL: D^T D w = 0; g_given: Gy
// holds g itself, the test entry's prescribed vector); kappa_j = kvec ? kvec[j] * kscale : kappa.  Per chunk c:
// vpart[c] / ipart[c] = the largest |g_j| - kappa_j over the columns j < d outside S and its column (ties: the smaller),
// qpart[c] = max |q_j|.
__global__ __launch_bounds__(OP_THREADS) void k_ws_scan(long long ld, long long d, long long nchunks, const double* __restrict__ Gy,
                                                       int g_given, const double* __restrict__ w, const double* __restrict__ q,
                                                       const double* __restrict__ l2, double rho, const double* __restrict__ kvec,
                                                       double kscale, double kappa, const int* __restrict__ pos,
                                                       double* __restrict__ vpart, int* __restrict__ ipart,
                                                       double* __restrict__ qpart) {
    __shared__ double sv[OP_THREADS / 64];
    __shared__ int si[OP_THREADS / 64];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double best = WS_NONE, qm = 0.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j0 = op_packet(c, (int)threadIdx.x, k);
            if (j0 < ld) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const long long j = j0 + e;
                    const double qq = q ? q[j] : 0.0;
                    qm = fmax(qm, fabs(qq));
                    if (j < d && pos[j] < 0) {
                        double g = Gy ? Gy[j] : 0.0;
                        if (!g_given) {
                            if (l2) g += (l2[j] / rho) * w[j];
                            g -= qq;
                        }
                        const double v = fabs(g) - (kvec ? kvec[j] * kscale : kappa);
                        ws_better(best, bi, v, (int)j);
                    }
                }
            }
        }
        ws_block_argmax(best, bi, sv, si);
        double qv = qm;
        int dummy = 0;
        ws_block_argmax(qv, dummy, sv, si);
        if (threadIdx.x == 0) {
            vpart[c] = best;
            ipart[c] = bi;
            qpart[c] = qv;
        }
    }
}

// One block: thr = tol * max(1, max_c qpart[c]); up to `take` chunk winners above thr, largest first, ties to the smaller
// column, go to the pinned block: pin[1] = how many, pin[2] = info[0] (the support size k_ws_scatter counted), pin[3] =
// candidates in all, pin[4 ..] = the columns, pin[0] = seq last.  vpart is consumed.
__global__ __launch_bounds__(OP_THREADS) void k_ws_select(long long nchunks, double* __restrict__ vpart, const int* __restrict__ ipart,
                                                         const double* __restrict__ qpart, double tol, int take,
                                                         const int* __restrict__ info, int* __restrict__ pin, int seq) {
    __shared__ double sv[OP_THREADS / 64];
    __shared__ int si[OP_THREADS / 64];
    double qv = 0.0;
    int dummy = 0;
    for (long long c = threadIdx.x; c < nchunks; c += OP_THREADS) qv = fmax(qv, qpart[c]);
    ws_block_argmax(qv, dummy, sv, si);
    const double thr = tol * fmax(1.0, qv);
    int ncand = 0;
    for (long long c = threadIdx.x; c < nchunks; c += OP_THREADS) ncand += vpart[c] > thr;
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    if (ncand) atomicAdd(&tot, ncand);
    __syncthreads();
    int n = 0;
    for (; n < take; ++n) {
        double best = WS_NONE;
        int bi = 0x7fffffff;
        for (long long c = threadIdx.x; c < nchunks; c += OP_THREADS) ws_better(best, bi, vpart[c], ipart[c]);
        ws_block_argmax(best, bi, sv, si);
        if (!(best > thr)) break;   // (the block's: every thread holds the same pair)
        if (threadIdx.x == 0) {
            pin[4 + n] = bi;
            vpart[bi / OP_CHUNK] = WS_NONE;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pin[1] = n;
        pin[2] = info ? info[0] : 0;
        pin[3] = tot;
        __threadfence_system();
        reinterpret_cast<volatile int*>(pin)[0] = seq;
    }
}

int ws_launch_scan(int64_t ld, int64_t d, const double* Gy, int g_given, const double* w, const double* q, const double* l2,
                   double rho, const double* kvec, double kscale, double kappa, double tol, int take, WsetState& W,
                   hipStream_t s) {
    const long long nc = op_num_chunks(ld);
    W.seq = (W.seq & 0x3fffffff) + 1;
    reinterpret_cast<volatile int*>(W.pin)[0] = 0;
    hipLaunchKernelGGL(k_ws_scan, dim3(op_grid(nc)), dim3(OP_THREADS), 0, s, (long long)ld, (long long)d, nc, Gy, g_given, w, q, l2, rho,
                       kvec, kscale, kappa, (const int*)W.pos, W.vpart, W.ipart, W.qpart);
    hipLaunchKernelGGL(k_ws_select, dim3(1), dim3(OP_THREADS), 0, s, nc, W.vpart, (const int*)W.ipart, (const double*)W.qpart, tol,
                       take < WS_SELECT ? take : WS_SELECT, (const int*)W.info, W.pin, W.seq);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

// the verdict of the scan in flight: the host's one wait of a round beside the restricted solve's
int ws_wait_scan(WsetState& W, hipStream_t s) {
    rbl_spin_wait(W.pin, 0, s);
    if (reinterpret_cast<const volatile int*>(W.pin)[0] != W.seq) {
        rbl_set_error("w-step (working set): the scan did not complete");
        (void)hipGetLastError();
        return RBL_ERR_HIP;
    }
    return RBL_OK;
}

// appends cols to S on the host and the device and forms their rows of Gs (batches of WS_SELECT)
int ws_add(const CsrStore* st, WsetState& W, const int* cols, int n, bool fixed, hipStream_t s) {
    for (int k0 = 0; k0 < n; k0 += WS_SELECT) {
        WsCols c;
        c.n = n - k0 < WS_SELECT ? n - k0 : WS_SELECT;
        for (int i = 0; i < WS_SELECT; ++i) c.col[i] = i < c.n ? cols[k0 + i] : 0;
        const int first = W.plan.add(c.col, c.n, fixed);
        if (first < 0) {
            rbl_set_error("w-step (working set): a column list the working set cannot take (internal)");
            return RBL_ERR_STATE;
        }
        hipLaunchKernelGGL(k_ws_append, dim3(1), dim3(WS_SELECT), 0, s, c, first, W.S, W.pos);
        // one block of four waves per compute unit at most (never fewer blocks than a batch of WS_SELECT needs on a whole
        // device; a test's num_cu = 1 makes the waves walk several columns each)
        int blocks = (c.n + WG_WPB - 1) / WG_WPB;
        if (blocks > W.num_cu) blocks = W.num_cu > 0 ? W.num_cu : 1;
        hipLaunchKernelGGL(k_ws_gram_rows, dim3((unsigned)blocks), dim3(WG_THREADS),
                           sizeof(double) * WG_WPB * WS_CAP, s, (const int64_t*)st->indptr, (const int*)st->col, (const double*)st->val,
                           (const int64_t*)st->colptr, (const int*)st->row, (const double*)st->cval, (const int*)W.pos, (const int*)W.S,
                           first, c.n, W.Gs);
        RBL_HIP(hipGetLastError());
        W.rep.rows_last += c.n;
        W.rep.rows_total += c.n;
    }
    return RBL_OK;
}

int ws_cap(int cap) { return cap < 1 ? 1 : cap > WS_CAP ? WS_CAP : cap; }

// S, pos, Gs empty (a first w-step, a new data epoch, a support S cannot be grown to)
int ws_clear(WsetState& W, int64_t ld, int cap, hipStream_t s) {
    W.plan.reset(ld, cap);
    W.rep.rows_total = 0;
    W.rep.evictions = 0;
    RBL_HIP(hipMemsetAsync(W.Gs, 0, sizeof(double) * (size_t)WS_CAP * WS_CAP, s));
    RBL_HIP(hipMemsetAsync(W.pos, 0xff, sizeof(int) * (size_t)ld, s));
    RBL_HIP(hipMemsetAsync(W.S, 0, sizeof(int) * WS_CAP, s));
    return RBL_OK;
}

// The working set is made to hold the free coordinates and the support of the w at hand (a first w-step, a w set from
// outside, a w-step that left the route): one blocking copy of w - not the steady state.  A support that does not fit
// beside S: S is rebuilt from it; one that does not fit at all: w <- 0, the cold start (a warm start is only that).
// left_before: the w-step before this one left the route - a support that still does not fit is not worth a cold start
// (*leave_now: go on with FISTA at once; the working set tries again once the support fits).
int ws_sync_support(const CsrStore* st, WsetState& W, int64_t ld, int64_t d, int cap, const double* l1_host, double* w,
                    bool left_before, bool* leave_now, hipStream_t s) {
    *leave_now = false;
    std::vector<double> hw((size_t)ld);
    RBL_HIP(hipMemcpyAsync(hw.data(), w, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
    RBL_HIP(hipStreamSynchronize(s));
    rbl_note_host_sync();
    std::vector<int> fr, sup;
    for (int64_t j = 0; j < d; ++j) {
        if (l1_host && l1_host[j] == 0.0) fr.push_back((int)j);
        else if (hw[(size_t)j] != 0.0) sup.push_back((int)j);
    }
    if (!W.built || W.plan.cap != ws_cap(cap)) {
        RBL_TRY(ws_clear(W, ld, cap, s));
        W.built = true;
    }
    auto missing = [&](const std::vector<int>& v) {
        std::vector<int> out;
        for (int j : v)
            if (!W.plan.has(j)) out.push_back(j);
        return out;
    };
    std::vector<int> mf = missing(fr), ms = missing(sup);
    if ((int64_t)mf.size() + (int64_t)ms.size() > W.plan.room()) {
        RBL_TRY(ws_clear(W, ld, cap, s));
        mf = fr;
        ms = sup;
        if ((int64_t)mf.size() > W.plan.room()) {
            *leave_now = true;   // more free coordinates than slots: S cannot hold what it must - the operator FISTA, form 4
            return RBL_OK;
        }
        if ((int64_t)mf.size() + (int64_t)ms.size() > W.plan.room()) {
            if (left_before) {
                *leave_now = true;
                return RBL_OK;   // (S stays empty and marked for a resync)
            }
            RBL_HIP(hipMemsetAsync(w, 0, sizeof(double) * (size_t)ld, s));
            ms.clear();
        }
    }
    RBL_TRY(ws_add(st, W, mf.data(), (int)mf.size(), true, s));
    RBL_TRY(ws_add(st, W, ms.data(), (int)ms.size(), false, s));
    W.resync = false;
    W.after_leave = false;
    return RBL_OK;
}

// the slots with w = 0 that are not free coordinates leave S; Gs is compacted into the spare buffer (one blocking copy
// of w_S: S was full, not the steady state)
int ws_evict(WsetState& W, hipStream_t s) {
    const int m = W.plan.size();
    std::vector<double> hw((size_t)(m > 0 ? m : 1));
    RBL_HIP(hipMemcpyAsync(hw.data(), W.wS, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s));
    RBL_HIP(hipStreamSynchronize(s));
    rbl_note_host_sync();
    std::vector<int> keep;
    const int gone = W.plan.evict(hw.data(), keep);
    if (gone == 0) return RBL_OK;
    if (!W.Gs2) RBL_TRY(W.mem->alloc(&W.Gs2, (size_t)WS_CAP * WS_CAP));
    const unsigned gb = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(k_ws_setpos, dim3(gb), dim3(256), 0, s, (const int*)W.S, m, 0, W.pos);
    const int m_new = W.plan.size();
    if (m_new > 0) RBL_HIP(hipMemcpyAsync(W.keep, keep.data(), sizeof(int) * (size_t)m_new, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ws_compact, dim3(WS_CAP * WS_CAP / 256), dim3(256), 0, s, (const double*)W.Gs, W.Gs2, (const int*)W.keep, m_new);
    if (m_new > 0) RBL_HIP(hipMemcpyAsync(W.S, W.plan.S.data(), sizeof(int) * (size_t)m_new, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ws_setpos, dim3(gb), dim3(256), 0, s, (const int*)W.S, m_new, 1, W.pos);
    RBL_HIP(hipGetLastError());
    RBL_HIP(hipStreamSynchronize(s));   // keep / plan.S are host vectors that go out of scope or move
    std::swap(W.Gs, W.Gs2);
    W.rep.evictions += gone;
    return RBL_OK;
}

}  // namespace

int alloc_wset(DevArena& mem, WsetState& W, int64_t ld, hipStream_t s, bool scan_only) {
    W.mem = &mem;
    const size_t nc = (size_t)op_num_chunks(ld);
    RBL_TRY(mem.alloc(&W.pos, (size_t)ld));
    RBL_TRY(mem.alloc(&W.vpart, 2 * nc));
    W.qpart = W.vpart + nc;
    RBL_TRY(mem.alloc(&W.ipart, nc));
    RBL_TRY(mem.alloc(&W.info, 4));
    RBL_HIP(hipMemsetAsync(W.info, 0, 4 * sizeof(int), s));
    RBL_TRY(mem.pinned(&W.pin, 4 + WS_SELECT, hipHostMallocCoherent));
    for (int i = 0; i < 4 + WS_SELECT; ++i) W.pin[i] = 0;
    W.rep = rbl_wset_report{};
    if (scan_only) return RBL_OK;   // (rbl_k_wset_scan: pos, the chunk partials and the pinned block are all it uses)
    RBL_TRY(mem.alloc(&W.Gs, (size_t)WS_CAP * WS_CAP));
    RBL_TRY(mem.alloc(&W.S, (size_t)WS_CAP));
    RBL_TRY(mem.alloc(&W.keep, (size_t)WS_CAP));
    RBL_TRY(mem.alloc(&W.qS, (size_t)4 * WS_CAP));
    W.wS = W.qS + WS_CAP;
    W.l1S = W.qS + 2 * WS_CAP;
    W.l2S = W.qS + 3 * WS_CAP;
    RBL_TRY(alloc_wstep(mem, W.small, WS_CAP, s));
    // device memory: Gs, the slot vectors, the chunk partials, pos / S / keep / the scan's columns, and the restricted
    // problem's workspace as alloc_wstep sizes it (five vectors, scalars, flags, the persistent kernels' words); the two
    // pinned blocks are host memory
    W.bytes = (int64_t)(sizeof(double) * ((size_t)WS_CAP * WS_CAP + 4 * WS_CAP + 2 * nc) + sizeof(int) * ((size_t)ld + 2 * WS_CAP + nc + 4) +
                        sizeof(double) * (5 * (size_t)WS_CAP + 8 + WSTEP_XCH_DOUBLES) + sizeof(int) * 8 + sizeof(unsigned) * WSTEP_BAR_UINTS);
    W.built = false;
    W.resync = true;
    return RBL_OK;
}

int wset_gram(const CsrStore* st, WsetState& W, int64_t ld, const int* cols, int n, int num_cu, hipStream_t s) {
    W.num_cu = num_cu;
    if (!W.built) {
        RBL_TRY(ws_clear(W, ld, WS_CAP, s));
        W.built = true;
    }
    return ws_add(st, W, cols, n, false, s);
}

int wset_scan(WsetState& W, int64_t ld, int64_t d, const double* g, const double* q, const double* kvec, const int* member_pos,
              double tol, int take, int* count, int* cols, hipStream_t s) {
    RBL_HIP(hipMemcpyAsync(W.pos, member_pos, sizeof(int) * (size_t)ld, hipMemcpyHostToDevice, s));
    RBL_TRY(ws_launch_scan(ld, d, g, 1, nullptr, q, nullptr, 1.0, kvec, 1.0, 0.0, tol, take, W, s));
    RBL_TRY(ws_wait_scan(W, s));
    const volatile int* pin = W.pin;
    *count = pin[1];
    for (int i = 0; i < *count; ++i) cols[i] = pin[4 + i];
    return RBL_OK;
}

int run_wstep_ws(const OpData& op, int64_t ld, int64_t d, const double* q, double rho, double reg, double L, double tol,
                 int max_inner, double* w, WstepWorkspace& ws, WsetState& W, int cap, const double* l1_host, int* iters_host,
                 hipStream_t s) {
    ws.gw_valid = false;
    ws.form = 5;
    if (!op.st || !op.t || !op.part || !op.slab || !op.st->colptr || !op.st->row || !op.st->cval || !op.st->lanes) {
        rbl_set_error("w-step (working set): the handle has no operator workspace, or its data are not complete");
        return RBL_ERR_STATE;
    }
    const bool pen = ws.pen_l1 != nullptr;
    if (pen) reg = 0.0;
    W.num_cu = op.num_cu;
    const bool left_before = W.after_leave;
    W.rep.rounds = W.rep.pass_pairs = W.rep.rows_last = W.rep.fista_on_gs = W.rep.left_route = 0;
    bool leave = false;
    if (!W.built || W.resync || W.plan.cap != ws_cap(cap))
        RBL_TRY(ws_sync_support(op.st, W, ld, d, cap, pen ? l1_host : nullptr, w, left_before, &leave, s));
    W.small.pen_l1 = pen ? W.l1S : nullptr;
    W.small.pen_l2 = pen ? W.l2S : nullptr;
    W.small.pen_l2max = ws.pen_l2max;
    W.small.eig_ok = false;
    W.small.inst = nullptr;
    int iters = 0, support = 0;
    for (int round = 0; !leave; ++round) {
        if (round >= WS_MAX_ROUNDS) {
            leave = true;
            break;
        }
        W.rep.rounds = round + 1;
        const int m = W.plan.size();
        // 1. the restricted problem on (Gs, q_S): the Gram route's l1 w-step, unchanged
        hipLaunchKernelGGL(k_ws_gather, dim3(WS_CAP / 256), dim3(256), 0, s, (const int*)W.S, m, q, (const double*)w, ws.pen_l1,
                           ws.pen_l2, W.qS, W.wS, W.l1S, W.l2S);
        RBL_HIP(hipGetLastError());
        int it = 0;
        RBL_TRY(run_wstep(RBL_WSTEP_L1, W.Gs, WS_CAP, W.qS, rho, reg, 1.0, L, tol, max_inner, W.wS, W.small, &it, s));
        iters += it;
        const bool exact = W.small.form == 2;
        if (!exact) W.rep.fista_on_gs = 1;
        const bool zero = exact && reinterpret_cast<const volatile int*>(W.small.pin)[3] == 0;   // the kernel's support size
        hipLaunchKernelGGL(k_ws_scatter, dim3(1), dim3(WG_THREADS), 0, s, (const int*)W.S, m, (const double*)W.wS, w, W.info);
        // 2. the scan over all columns
        if (!zero) {
            RBL_TRY(launch_csr_gemv(op.st, op.n, w, op.t, op.num_cu, s));
            RBL_TRY(launch_csr_gemvt(op.st, ld, op.t, op.slab, op.slab_doubles, ws.Gy, op.num_cu, s, nullptr));
            W.rep.pass_pairs += 1;
        }
        RBL_TRY(ws_launch_scan(ld, d, zero ? nullptr : ws.Gy, 0, w, q, pen ? ws.pen_l2 : nullptr, rho, ws.pen_l1, 1.0 / (2.0 * rho),
                               reg / (2.0 * rho), tol, WS_SELECT, W, s));
        RBL_TRY(ws_wait_scan(W, s));
        const volatile int* pin = W.pin;
        const int cnt = pin[1];
        support = pin[2];
        if (cnt == 0) break;   // the KKT conditions hold on all columns
        // 3. grow
        int cols[WS_SELECT];
        for (int i = 0; i < cnt; ++i) cols[i] = pin[4 + i];
        if (W.plan.room() < cnt) RBL_TRY(ws_evict(W, s));
        if (W.plan.room() == 0) {
            leave = true;
            break;
        }
        RBL_TRY(ws_add(op.st, W, cols, cnt < W.plan.room() ? cnt : W.plan.room(), false, s));
    }
    if (leave) {
        // S cannot hold what it must: FISTA on the operator from the current w; the next w-step finds its support again
        W.rep.left_route = 1;
        W.resync = true;
        W.after_leave = true;
        int it = 0;
        RBL_TRY(run_wstep_op(RBL_WSTEP_L1, op, ld, q, rho, reg, L, tol, max_inner, w, ws, &it, s));   // (ws.form = 4)
        iters += it;
        support = -1;
    }
    W.rep.slots = W.plan.size();
    W.rep.support = support;
    W.rep.form = ws.form;
    W.rep.bytes = W.bytes + (W.Gs2 ? (int64_t)sizeof(double) * WS_CAP * WS_CAP : 0);
    if (iters_host) *iters_host = iters;
    return RBL_OK;
}
