// wstep_op.hip - the w-sub-problem without the Gram matrix (RBL_CREATE_NO_GRAM, storage RBL_STORE_CSR), fp64.
//
// wstep.hip works on G = D^T D, an ld x ld matrix: 80 GB at d = 100 000.  Here A = rho D^T D + diag(.) is applied as an
// operator, A p = rho D^T (D p) + reg p + l2 .* p, with the two sparse passes of spmv.hip (t = D p into an n-vector,
// y = D^T t through the segment slab): nothing of size d^2 exists.  Borrowers with labels of their own have D_k = r .* D,
// r = +-1, so D_k^T D_k = D^T D: the operator is the owner's.
//   ridge:  warm-started CG on (rho D^T D + reg I + diag(l2)) w = rho q - the recurrences, the stop rule r'r <= tol^2
//           ||rho q||^2 and the alpha == 0 exit of k_cg_init / k_cg_update (wstep.hip), batched as run_wstep batches them;
//   lasso / elastic net:  FISTA with gradient restart, step 1/L, per-coordinate thresholds - the update and the stop rule
//           max |dw| <= tol max(1, max |w|) of k_fista_update<PEN>.  The active-set kernel needs G and is not used.
// The d-space kernels are multi-block for any d: a vector is cut into chunks (wstep_op_plan.h), every sum and maximum is
// one partial per chunk in a fixed order, and every block of the consuming kernel re-adds the partials in chunk order.
// The grid enters no bit of a result; there are no float atomics.  The padding [d, ld) of w, r, p, y stays +0.0.
//
// An iteration's scalars (r'r, FISTA's t) alternate between two slots by the iteration's parity: the kernel that closes
// an iteration writes the slot its blocks do not read.  For the same reason it does not test the word it sets: flags[0]
// (done) is set by the closing kernel and read by the kernels in front of it, whose first block copies it to flags[2],
// the word the closing kernel tests.  After convergence every launch of a batch is a no-op, the sparse passes included
// (they take flags[0] as their optional done flag).
#include "rbl_internal.h"
#include "device_math.h"
#include "wstep_op_plan.h"

namespace {

// scal: [3] ||y|| of the power iteration, [2] CG's threshold on r'r, [4 + parity] r'r, [6 + parity] FISTA's t
// flags: [0] done, [1] iterations, [2] done as the iteration in flight found it
constexpr int SC_NORM = 3, SC_THR = 2, SC_RR = 4, SC_T = 6;

__device__ inline double2 ld2(const double* p, long long j) { return *reinterpret_cast<const double2*>(p + j); }
__device__ inline void st2(double* p, long long j, double a, double b) { *reinterpret_cast<double2*>(p + j) = make_double2(a, b); }

// the partials of a sum / a maximum, added in chunk order (every thread of every block: the same bits everywhere)
__device__ inline double op_total(const double* __restrict__ part, long long nchunks) {
    double s = 0.0;
    for (long long c = 0; c < nchunks; ++c) s += part[c];
    return s;
}
__device__ inline double op_total_max(const double* __restrict__ part, long long nchunks) {
    double m = 0.0;
    for (long long c = 0; c < nchunks; ++c) m = fmax(m, part[c]);
    return m;
}

template <int K>
__device__ inline void block_max(double (&val)[K], double* smem /* K * OP_THREADS / 64 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) val[k] = fmax(val[k], __shfl_xor(val[k], off, 64));
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) smem[wave * K + k] = val[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double m = smem[k];
        for (int w = 1; w < OP_THREADS / 64; ++w) m = fmax(m, smem[w * K + k]);
        val[k] = m;
    }
}

__device__ inline double soft_thr(double b, double k) {   // src/util/fast_lasso.py:15-19
    const double a = fabs(b) - k;
    return a > 0.0 ? copysign(a, b) : 0.0;
}

// the start vector of launch_power_iteration (wstep.hip: k_power_init)
__global__ void k_op_power_init(long long ld, long long d, double* __restrict__ x) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < ld; j += (long long)gridDim.x * blockDim.x) {
        unsigned long long h = (unsigned long long)(j + 1) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        x[j] = (j < d) ? 0.5 + (double)(h & 0xffff) / 65536.0 : 0.0;
    }
}

// part[c] = sum of y^2 over chunk c
__global__ __launch_bounds__(OP_THREADS) void k_op_sumsq(long long ld, long long nchunks, const double* __restrict__ y,
                                                        double* __restrict__ part) {
    __shared__ double smem[OP_THREADS / 64];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 a = ld2(y, j);
                acc[0] += a.x * a.x;
                acc[0] += a.y * a.y;
            }
        }
        rbl::block_sum<1, OP_THREADS>(acc, smem);
        if (threadIdx.x == 0) part[c] = acc[0];
    }
}

// x <- y / ||y|| ; scal[SC_NORM] = ||y||   (k_normalize of wstep.hip, on the partials of k_op_sumsq)
// (x may be y itself: no __restrict__ on the two)
__global__ __launch_bounds__(OP_THREADS) void k_op_scale(long long ld, long long nchunks, const double* y, double* x,
                                                        const double* __restrict__ part, double* __restrict__ scal) {
    const double nrm = sqrt(op_total(part, nchunks));
    const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 a = ld2(y, j);
                st2(x, j, a.x * inv, a.y * inv);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[SC_NORM] = nrm;
}

// y holds D^T D p:  y <- rho y + reg p (l2 == NULL) or rho y + l2 .* p;  part[c] = sum of p y over chunk c.
// First d-space kernel of a CG iteration (flags != NULL): a no-op once done, and its first block notes what it found.
__global__ __launch_bounds__(OP_THREADS) void k_op_apply(long long ld, long long nchunks, const double* __restrict__ p,
                                                        double* __restrict__ y, double rho, double reg,
                                                        const double* __restrict__ l2, double* __restrict__ part,
                                                        int* __restrict__ flags) {
    if (flags) {
        const int done = flags[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) flags[2] = done;
        if (done) return;
    }
    __shared__ double smem[OP_THREADS / 64];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 a = ld2(y, j), b = ld2(p, j);
                double2 dg = make_double2(reg, reg);
                if (l2) dg = ld2(l2, j);
                const double y0 = rho * a.x + dg.x * b.x, y1 = rho * a.y + dg.y * b.y;
                st2(y, j, y0, y1);
                acc[0] += b.x * y0;
                acc[0] += b.y * y1;
            }
        }
        rbl::block_sum<1, OP_THREADS>(acc, smem);
        if (threadIdx.x == 0) part[c] = acc[0];
    }
}

// r = p = rho q - A w;  part[c] = sum r^2, part[nchunks + c] = sum (rho q)^2   (k_cg_init of wstep.hip)
__global__ __launch_bounds__(OP_THREADS) void k_op_cg_init(long long ld, long long nchunks, const double* __restrict__ Aw,
                                                          const double* __restrict__ q, double rho, double* __restrict__ r,
                                                          double* __restrict__ p, double* __restrict__ part) {
    __shared__ double smem[2 * OP_THREADS / 64];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc[2] = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 a = ld2(Aw, j), b = ld2(q, j);
                const double b0 = rho * b.x, b1 = rho * b.y;
                const double r0 = b0 - a.x, r1 = b1 - a.y;
                st2(r, j, r0, r1);
                st2(p, j, r0, r1);
                acc[0] += r0 * r0;
                acc[0] += r1 * r1;
                acc[1] += b0 * b0;
                acc[1] += b1 * b1;
            }
        }
        rbl::block_sum<2, OP_THREADS>(acc, smem);
        if (threadIdx.x == 0) {
            part[c] = acc[0];
            part[nchunks + c] = acc[1];
        }
    }
}

// ... and its scalars: r'r (slot 0), the threshold, done, the iteration count
__global__ void k_op_cg_init_fin(long long nchunks, const double* __restrict__ part, double tol, double* __restrict__ scal,
                                 int* __restrict__ flags) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double rr = op_total(part, nchunks), bb = op_total(part + nchunks, nchunks);
    scal[SC_RR] = rr;
    scal[SC_THR] = tol * tol * bb;
    flags[0] = (rr <= scal[SC_THR]) ? 1 : 0;
    flags[1] = 0;
    flags[2] = flags[0];
}

// first half of k_cg_update: alpha = r'r / p'Ap;  w += alpha p, r -= alpha A p;  partR[c] = sum of the new r^2
__global__ __launch_bounds__(OP_THREADS) void k_op_cg_wr(long long ld, long long nchunks, const double* __restrict__ Ap,
                                                        double* __restrict__ w, double* __restrict__ r,
                                                        const double* __restrict__ p, const double* __restrict__ scal,
                                                        const int* __restrict__ flags, int par,
                                                        const double* __restrict__ partA, double* __restrict__ partR) {
    if (flags[2]) return;
    __shared__ double smem[OP_THREADS / 64];
    const double pAp = op_total(partA, nchunks);
    const double rr = scal[SC_RR + par];
    const double alpha = (pAp > 0.0) ? rr / pAp : 0.0;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 a = ld2(Ap, j), pk = ld2(p, j), wk = ld2(w, j), rk = ld2(r, j);
                st2(w, j, wk.x + alpha * pk.x, wk.y + alpha * pk.y);
                const double r0 = rk.x - alpha * a.x, r1 = rk.y - alpha * a.y;
                st2(r, j, r0, r1);
                acc[0] += r0 * r0;
                acc[0] += r1 * r1;
            }
        }
        rbl::block_sum<1, OP_THREADS>(acc, smem);
        if (threadIdx.x == 0) partR[c] = acc[0];
    }
}

// second half: beta = r'r new / r'r;  p = r + beta p;  the first block closes the iteration (done, count, publish)
__global__ __launch_bounds__(OP_THREADS) void k_op_cg_p(long long ld, long long nchunks, const double* __restrict__ r,
                                                       double* __restrict__ p, double* __restrict__ scal,
                                                       int* __restrict__ flags, int par, const double* __restrict__ partA,
                                                       const double* __restrict__ partR, int* __restrict__ publish) {
    // publish != NULL on the last update of a batch: (done, iterations) go to pinned host memory, word 0 last
    if (flags[2]) {
        if (publish && blockIdx.x == 0 && threadIdx.x == 0) {
            publish[1] = flags[1];
            __threadfence_system();
            publish[0] = 1;
        }
        return;
    }
    const double rr_new = op_total(partR, nchunks);
    const double rr = scal[SC_RR + par];
    const double beta = (rr > 0.0) ? rr_new / rr : 0.0;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 rk = ld2(r, j), pk = ld2(p, j);
                st2(p, j, rk.x + beta * pk.x, rk.y + beta * pk.y);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double pAp = op_total(partA, nchunks);
        const double alpha = (pAp > 0.0) ? rr / pAp : 0.0;
        scal[SC_RR + (par ^ 1)] = rr_new;
        const int it = flags[1] + 1;
        const int done = (rr_new <= scal[SC_THR] || alpha == 0.0) ? 1 : 0;
        flags[1] = it;
        if (done) flags[0] = 1;
        if (publish) {
            publish[1] = it;
            __threadfence_system();
            publish[0] = done;
        }
    }
}

struct OpFista {
    double L;       // step constant of the smooth part (max_j l2_j / rho included)
    double kappa;   // reg / (2 rho), the threshold without per-coordinate penalties
    double rho;
};

// first half of k_fista_update<PEN>: the prox point x of the extrapolated y goes to wn; per chunk the restart sum
// (y - x)(x - w) and the two maxima |x - w|, |x|.  Gy holds D^T D yk
__global__ __launch_bounds__(OP_THREADS) void k_op_fista_x(long long ld, long long nchunks, const double* __restrict__ Gy,
                                                          const double* __restrict__ q, const double* __restrict__ w,
                                                          const double* __restrict__ yk, double* __restrict__ wn, OpFista P,
                                                          const double* __restrict__ l1, const double* __restrict__ l2,
                                                          int* __restrict__ flags, double* __restrict__ part) {
    const int done = flags[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[2] = done;
    if (done) return;
    __shared__ double smem[2 * OP_THREADS / 64];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc[1] = {0.0};
        double mx[2] = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 g = ld2(Gy, j), qq = ld2(q, j), y = ld2(yk, j), wk = ld2(w, j);
                double b0, b1, k0 = P.kappa / P.L, k1 = k0;
                if (l1) {   // (uniform: per-coordinate penalties, l2 given with them)
                    const double2 a1 = ld2(l1, j), a2 = ld2(l2, j);
                    b0 = y.x - (g.x + (a2.x / P.rho) * y.x - qq.x) / P.L;
                    b1 = y.y - (g.y + (a2.y / P.rho) * y.y - qq.y) / P.L;
                    k0 = a1.x / (2.0 * P.rho) / P.L;
                    k1 = a1.y / (2.0 * P.rho) / P.L;
                } else {
                    b0 = y.x - (g.x - qq.x) / P.L;
                    b1 = y.y - (g.y - qq.y) / P.L;
                }
                const double x0 = soft_thr(b0, k0), x1 = soft_thr(b1, k1);
                const double d0 = x0 - wk.x, d1 = x1 - wk.y;
                st2(wn, j, x0, x1);
                acc[0] += (y.x - x0) * d0;
                acc[0] += (y.y - x1) * d1;
                mx[0] = fmax(mx[0], fmax(fabs(d0), fabs(d1)));
                mx[1] = fmax(mx[1], fmax(fabs(x0), fabs(x1)));
            }
        }
        rbl::block_sum<1, OP_THREADS>(acc, smem);
        block_max<2>(mx, smem);
        if (threadIdx.x == 0) {
            part[c] = acc[0];
            part[nchunks + c] = mx[0];
            part[2 * nchunks + c] = mx[1];
        }
    }
}

// second half: restart test, t, w <- x, yk <- x + coef (x - w);  the first block closes the iteration
__global__ __launch_bounds__(OP_THREADS) void k_op_fista_upd(long long ld, long long nchunks, double* __restrict__ w,
                                                            double* __restrict__ yk, const double* __restrict__ wn,
                                                            double* __restrict__ scal, int* __restrict__ flags, int par,
                                                            const double* __restrict__ part, double tol,
                                                            int* __restrict__ publish) {
    if (flags[2]) {
        if (publish && blockIdx.x == 0 && threadIdx.x == 0) {
            publish[1] = flags[1];
            __threadfence_system();
            publish[0] = 1;
        }
        return;
    }
    const double acc = op_total(part, nchunks);
    const double mx_dw = op_total_max(part + nchunks, nchunks), mx_w = op_total_max(part + 2 * nchunks, nchunks);
    const double t = scal[SC_T + par];
    const bool restart = acc > 0.0;   // O'Donoghue-Candes gradient restart
    const double tn = restart ? 1.0 : 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
    const double coef = restart ? 0.0 : (t - 1.0) / tn;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < OP_PACKETS; ++k) {
            const long long j = op_packet(c, (int)threadIdx.x, k);
            if (j < ld) {
                const double2 x = ld2(wn, j), wk = ld2(w, j);
                st2(w, j, x.x, x.y);
                st2(yk, j, x.x + coef * (x.x - wk.x), x.y + coef * (x.y - wk.y));
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[SC_T + (par ^ 1)] = tn;
        const int it = flags[1] + 1;
        const int done = (mx_dw <= tol * fmax(1.0, mx_w)) ? 1 : 0;
        flags[1] = it;
        if (done) flags[0] = 1;
        if (publish) {
            publish[1] = it;
            __threadfence_system();
            publish[0] = done;
        }
    }
}

// y = D^T (D x): the two sparse passes, through the n-vector and the segment slab; no-ops where *done is set
int op_dtd(const OpData& op, int64_t ld, const double* x, double* y, hipStream_t s, const int* done = nullptr) {
    RBL_TRY(launch_csr_gemv(op.st, op.n, x, op.t, op.num_cu, s, done));
    return launch_csr_gemvt(op.st, ld, op.t, op.slab, op.slab_doubles, y, op.num_cu, s, nullptr, done);
}

int run_cg_op(const OpData& op, int64_t ld, const double* q, double rho, double reg, double tol, int max_inner, double* w,
              WstepWorkspace& ws, int* iters_host, hipStream_t s) {
    const long long nc = op_num_chunks(ld);
    const dim3 grid(op_grid(nc)), block(OP_THREADS);
    const double* l2 = ws.pen_l1 ? ws.pen_l2 : nullptr;
    double *partA = op.part, *partR = op.part + nc;   // (k_op_cg_init: both halves, before the first iteration)
    RBL_TRY(op_dtd(op, ld, w, ws.Gy, s));
    hipLaunchKernelGGL(k_op_apply, grid, block, 0, s, (long long)ld, nc, (const double*)w, ws.Gy, rho, reg, l2, op.part + 2 * nc,
                       (int*)nullptr);
    hipLaunchKernelGGL(k_op_cg_init, grid, block, 0, s, (long long)ld, nc, (const double*)ws.Gy, q, rho, ws.r, ws.p, op.part);
    hipLaunchKernelGGL(k_op_cg_init_fin, dim3(1), dim3(64), 0, s, nc, (const double*)op.part, tol, ws.scal, ws.flags);
    RBL_HIP(hipGetLastError());
    int batch = ws.last_iters > 0 ? ws.last_iters + 2 : 16;
    if (batch < 4) batch = 4;
    if (batch > 64) batch = 64;
    int done_iters = 0, done = 0, iters = 0;
    while (done_iters < max_inner) {
        ws.pin[4] = -1;
        for (int b = 0; b < batch; ++b) {
            const int par = (done_iters + b) & 1;
            RBL_TRY(op_dtd(op, ld, ws.p, ws.Gy, s, ws.flags));
            hipLaunchKernelGGL(k_op_apply, grid, block, 0, s, (long long)ld, nc, (const double*)ws.p, ws.Gy, rho, reg, l2, partA,
                               ws.flags);
            hipLaunchKernelGGL(k_op_cg_wr, grid, block, 0, s, (long long)ld, nc, (const double*)ws.Gy, w, ws.r, (const double*)ws.p,
                               (const double*)ws.scal, (const int*)ws.flags, par, (const double*)partA, partR);
            hipLaunchKernelGGL(k_op_cg_p, grid, block, 0, s, (long long)ld, nc, (const double*)ws.r, ws.p, ws.scal, ws.flags, par,
                               (const double*)partA, (const double*)partR, b == batch - 1 ? ws.pin + 4 : (int*)nullptr);
        }
        RBL_HIP(hipGetLastError());
        done_iters += batch;
        rbl_spin_wait(ws.pin + 4, -1, s);
        const volatile int* st = ws.pin + 4;
        done = st[0];
        iters = st[1];
        if (done != 0) break;   // 1 = converged (-1 after the spin's stream wait: launch failure, stop too)
        batch = 8;
    }
    if (done == 1) ws.last_iters = iters;
    if (iters_host) *iters_host = iters;
    if (done == -1) {
        rbl_set_error("w-step (operator route): the CG batch did not complete");
        return RBL_ERR_HIP;
    }
    return RBL_OK;
}

int run_fista_op(const OpData& op, int64_t ld, const double* q, double rho, double reg, double L, double tol, int max_inner,
                 double* w, WstepWorkspace& ws, int* iters_host, hipStream_t s) {
    constexpr int BATCH = 8;
    const long long nc = op_num_chunks(ld);
    const dim3 grid(op_grid(nc)), block(OP_THREADS);
    const bool pen = ws.pen_l1 != nullptr;
    OpFista P;
    P.L = pen ? L + ws.pen_l2max / rho : L;
    P.kappa = reg / (2.0 * rho);
    P.rho = rho;
    const double one[2] = {1.0, 1.0};
    RBL_HIP(hipMemcpyAsync(ws.scal + SC_T, one, 2 * sizeof(double), hipMemcpyHostToDevice, s));
    RBL_HIP(hipMemsetAsync(ws.flags, 0, 3 * sizeof(int), s));
    RBL_HIP(hipMemcpyAsync(ws.yk, w, sizeof(double) * ld, hipMemcpyDeviceToDevice, s));
    int batch = ws.last_fista > 0 ? ws.last_fista + ws.last_fista / 4 + 2 : 4 * BATCH;
    if (batch < BATCH) batch = BATCH;
    if (batch > 512) batch = 512;
    int done_iters = 0, done = 0, iters = 0;
    while (done_iters < max_inner) {
        ws.pin[6] = -1;
        for (int b = 0; b < batch; ++b) {
            const int par = (done_iters + b) & 1;
            RBL_TRY(op_dtd(op, ld, ws.yk, ws.Gy, s, ws.flags));
            hipLaunchKernelGGL(k_op_fista_x, grid, block, 0, s, (long long)ld, nc, (const double*)ws.Gy, q, (const double*)w,
                               (const double*)ws.yk, ws.wn, P, ws.pen_l1, pen ? ws.pen_l2 : (const double*)nullptr, ws.flags,
                               op.part);
            hipLaunchKernelGGL(k_op_fista_upd, grid, block, 0, s, (long long)ld, nc, w, ws.yk, (const double*)ws.wn, ws.scal,
                               ws.flags, par, (const double*)op.part, tol, b == batch - 1 ? ws.pin + 6 : (int*)nullptr);
        }
        RBL_HIP(hipGetLastError());
        done_iters += batch;
        rbl_spin_wait(ws.pin + 6, -1, s);
        const volatile int* st = ws.pin + 6;
        done = st[0];
        iters = st[1];
        if (done != 0) break;
        batch = 4 * BATCH;
    }
    if (done == 1) ws.last_fista = iters;
    if (iters_host) *iters_host = iters;
    if (done == -1) {
        rbl_set_error("w-step (operator route): the FISTA batch did not complete");
        return RBL_ERR_HIP;
    }
    return RBL_OK;
}

}  // namespace

size_t op_part_doubles(int64_t ld) { return (size_t)op_num_chunks(ld) * 3; }

int launch_op_power_iteration(const OpData& op, int64_t ld, int64_t d, double* x, double* y, double* scal, int iters,
                              double* lambda_host, hipStream_t s) {
    const long long nc = op_num_chunks(ld);
    const dim3 grid(op_grid(nc)), block(OP_THREADS);
    hipLaunchKernelGGL(k_op_power_init, dim3(64), dim3(256), 0, s, (long long)ld, (long long)d, x);
    hipLaunchKernelGGL(k_op_sumsq, grid, block, 0, s, (long long)ld, nc, (const double*)x, op.part);
    hipLaunchKernelGGL(k_op_scale, grid, block, 0, s, (long long)ld, nc, (const double*)x, x, (const double*)op.part, scal);
    for (int it = 0; it < iters; ++it) {
        RBL_TRY(op_dtd(op, ld, x, y, s));
        hipLaunchKernelGGL(k_op_sumsq, grid, block, 0, s, (long long)ld, nc, (const double*)y, op.part);
        hipLaunchKernelGGL(k_op_scale, grid, block, 0, s, (long long)ld, nc, (const double*)y, x, (const double*)op.part, scal);
    }
    RBL_HIP(hipGetLastError());
    RBL_HIP(hipMemcpyAsync(lambda_host, scal + SC_NORM, sizeof(double), hipMemcpyDeviceToHost, s));
    RBL_HIP(hipStreamSynchronize(s));
    return RBL_OK;
}

int run_wstep_op(int wstep, const OpData& op, int64_t ld, const double* q, double rho, double reg, double L, double tol,
                 int max_inner, double* w, WstepWorkspace& ws, int* iters_host, hipStream_t s) {
    ws.gw_valid = false;
    ws.form = 4;
    if (wstep == RBL_WSTEP_SMOOTH_L1) {
        rbl_set_error("w-step (operator route): the smoothed-l1 w-step preconditions with diag(G) and there is no Gram matrix "
                      "on this route");
        return RBL_ERR_INVALID;
    }
    if (!op.st || !op.t || !op.part || !op.slab) {
        rbl_set_error("w-step (operator route): the handle has no operator workspace");
        return RBL_ERR_STATE;
    }
    // per-coordinate penalties (rbl_set_penalty): ws.pen_l1 / ws.pen_l2 replace reg
    if (ws.pen_l1) reg = 0.0;
    if (wstep == RBL_WSTEP_L2) return run_cg_op(op, ld, q, rho, reg, tol, max_inner, w, ws, iters_host, s);
    return run_fista_op(op, ld, q, rho, reg, L, tol, max_inner, w, ws, iters_host, s);
}
