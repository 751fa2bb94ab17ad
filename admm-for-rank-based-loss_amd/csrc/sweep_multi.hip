// sweep_multi.hip - the two n x d passes of the ADMM iteration for SEVERAL problems on one data matrix:
//     V pass   v_k = D w_k,  lambda_k += rho_k (z_k - v_k),  sum (z_k - v_k)^2      (K-column form of SE_VONLY)
//     Q pass   q_k = D^T c_k                                                       (K-column form of SE_QONLY)
// for up to RBL_MULTI_KMAX columns per launch.  D is read ONCE per launch with the loads of k_sweep_erm
// (sweep_erm.hip): a wave owns R rows at a time, P 16-byte packets per lane and row through scalar row descriptors
// (buffer_load_dwordx4, non-temporal), the next sub-batch in flight while the current one is processed, S sub-batches to
// a super-batch whose row-wise state is read and written as whole lines.  The pass stays bound by the bytes of D; what
// grows with K is the arithmetic per packet (E x K fp64 FMAs) and
//   V pass: the LDS reads of w_k (K x ld doubles staged per block: 64 KB at K = 4, ld = 2048) - one read of w serves
//           the R rows of the sub-batch - and R x K wave reductions per sub-batch;
//   Q pass: K x P x E fp64 column sums per lane (K = 4, d = 1000 fp32: 128 doubles = 256 VGPRs beside the two row
//           buffers' 128 - one block of 4 waves per CU, up to 512 registers per lane).
// Shapes (P, R, S), the grid (one block per CU), the row -> wave assignment and the order of every fp64 sum are those of
// the single-column passes (launch_sweep_v / launch_sweep_q), so column k of a K-column launch is bit-identical to the
// single-column pass on the same inputs, and to itself from run to run: per-lane FMA chains in packet order, DPP
// butterfly, block sums in wave order, one slab row per block and column, two-stage fixed-order column reduction.
#include "rbl_internal.h"
#ifndef RBL_D_AUX
#define RBL_D_AUX 2   // cache policy of the streaming loads of D, as in sweep_erm.hip
#endif
#include "device_math.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Pk;
template <> struct Pk<float> {
    static constexpr int E = 4;
    __device__ static inline double at(const u32x4& p, int k) { return (double)__uint_as_float(p[k]); }
};
template <> struct Pk<double> {
    static constexpr int E = 2;
    __device__ static inline double at(const u32x4& p, int k) { return __hiloint2double((int)p[2 * k + 1], (int)p[2 * k]); }
};
// fp16 storage: element k is the low (k even) or high half of dword k / 2, widened half -> float -> double (both exact)
template <> struct Pk<rbl_half> {
    static constexpr int E = 8;
    __device__ static inline double at(const u32x4& p, int k) {
        const unsigned short h = (unsigned short)((k & 1) ? p[k >> 1] >> 16 : p[k >> 1]);
        return (double)(float)__builtin_bit_cast(_Float16, h);
    }
};

constexpr int SM_THREADS = 256;
constexpr int SM_SLICES = 8;   // slices of the column reduction (CR_SLICES of sweep_erm.hip: same order of the sums)

// row-wise results leave write-through, as in sweep_erm.hip (row_store)
__device__ inline void row_store(double* __restrict__ base, long long row, double x) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(base + row), __builtin_bit_cast(unsigned long long, x), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// the K columns of one launch; slots >= k repeat column 0 (read, never written)
struct MultiV {
    const double* w[RBL_MULTI_KMAX];
    const double* z[RBL_MULTI_KMAX];
    double* lam[RBL_MULTI_KMAX];
    double* v[RBL_MULTI_KMAX];
    double* partials[RBL_MULTI_KMAX];   // 3 doubles per block, slot 0 = sum (z - v)^2 (the layout k_sweep_erm writes)
    double rho[RBL_MULTI_KMAX];
    int k;
    int update;                         // 0: v = D w alone (no z / lambda access, no residual sums)
};
struct MultiQ {
    const double* c[RBL_MULTI_KMAX];
    double* q[RBL_MULTI_KMAX];
    int k;
};

// ---- V pass ------------------------------------------------------------------------------------------------------
template <typename T, int P, int R, int S, int KC>
__global__ __launch_bounds__(SM_THREADS, 1) void k_sweep_vm(const T* __restrict__ D, long long n, long long ld, MultiV a) {
    constexpr int E = Pk<T>::E;
    constexpr int CW = 64 * P * E;   // doubles of one staged w, laid out [p][lane][k] as in k_sweep_erm
    extern __shared__ __align__(16) double sw[];   // KC x CW
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int PK = (int)(ld / E);
    const unsigned row_bytes = (unsigned)ld * (unsigned)sizeof(T);
    const bool update = a.update != 0;

    int boff[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int pkp = lane + 64 * p;
        const bool ok = pkp < PK;
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c)
#pragma unroll
                for (int k = 0; k < E; ++k) sw[c * CW + (p * 64 + lane) * E + k] = ok ? a.w[c][(long long)pkp * E + k] : 0.0;
        }
        boff[p] = ok ? pkp * 16 : 0x7ffffff0;   // past the row end: outside the descriptor, the load returns 0
    }
    __syncthreads();
    double s_prim[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) s_prim[c] = 0.0;

    constexpr int SR = S * R;
    const int nsuper = (int)((n + SR - 1) / SR);
    const int live_last = (int)(n - (long long)(nsuper - 1) * SR);
    const int gw = (int)blockIdx.x * (SM_THREADS / 64) + wave;
    const int GW = (int)gridDim.x * (SM_THREADS / 64);

    auto load_side = [&](int q, double (&zo)[KC], double (&lm)[KC]) {
        const int live = q == nsuper - 1 ? live_last : SR;
        const bool mine = lane < live && update;
        const long long myrow = (long long)q * SR + lane;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            zo[c] = mine ? a.z[c][myrow] : 0.0;
            lm[c] = mine ? a.lam[c][myrow] : 0.0;
        }
    };
    auto load_rows = [&](int q, int sub, u32x4 (&buf)[R][P]) {
        const int live = q == nsuper - 1 ? live_last : SR;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int i = sub * R + r;
            if (i >= live) i = live - 1;   // rows past n re-read the last row; nothing of them is stored
            const long long row = (long long)q * SR + i;
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(D + row * ld), 0, (int)row_bytes, 0x00020000);
#pragma unroll
            for (int p = 0; p < P; ++p) buf[r][p] = __builtin_amdgcn_raw_buffer_load_b128(rs, boff[p], 0, RBL_D_AUX);
        }
    };

    double l_out[KC], v_out[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) l_out[c] = v_out[c] = 0.0;
    auto process = [&](int live, int sub, u32x4 (&buf)[R][P], const double (&zo)[KC], const double (&lm)[KC]) {
        double dot[R][KC];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < KC; ++c) dot[r][c] = 0.0;
        int woff = lane * E;
        asm volatile("" : "+v"(woff));   // keeps the loop-invariant LDS reads of w out of the registers
#pragma unroll
        for (int p = 0; p < P; ++p) {
            double wv[KC][E];
#pragma unroll
            for (int c = 0; c < KC; ++c)
#pragma unroll
                for (int k = 0; k < E; ++k) wv[c][k] = sw[c * CW + p * 64 * E + woff + k];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const double x = Pk<T>::at(buf[r][p], k);
#pragma unroll
                    for (int c = 0; c < KC; ++c) dot[r][c] = __builtin_fma(x, wv[c][k], dot[r][c]);
                }
        }
        const bool owner = lane >= sub * R && lane < sub * R + R && lane < live;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            double myv = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double d = rbl::wave_sum_all(dot[r][c]);
                myv = (lane == sub * R + r) ? d : myv;
            }
            if (owner) {
                const double res = zo[c] - myv;
                l_out[c] = lm[c] + a.rho[c] * res;   // algorithms.py:132
                s_prim[c] += res * res;               // algorithms.py:135
                v_out[c] = myv;
            }
        }
    };

    u32x4 bufA[R][P], bufB[R][P];
    double zo[KC], lm[KC], zoN[KC], lmN[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) zo[c] = lm[c] = zoN[c] = lmN[c] = 0.0;
    int q = gw, sub = 0;
    if (q < nsuper) {
        load_side(q, zoN, lmN);
        load_rows(q, 0, bufB);
    }
#pragma clang loop unroll(disable)
    while (q < nsuper) {
        const int live = q == nsuper - 1 ? live_last : SR;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int p = 0; p < P; ++p) bufA[r][p] = bufB[r][p];
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                zo[c] = zoN[c];
                lm[c] = lmN[c];
            }
        }
        const bool last = sub + 1 == S;
        const int qn = last ? q + GW : q;
        const int subn = last ? 0 : sub + 1;
        __builtin_amdgcn_sched_barrier(0);
        if (qn < nsuper) {
            if (last) load_side(qn, zoN, lmN);
            load_rows(qn, subn, bufB);
        }
        __builtin_amdgcn_sched_barrier(0);   // the prefetch stays above the arithmetic
        process(live, sub, bufA, zo, lm);
        if (last && lane < live) {
            const long long row = (long long)q * SR + lane;
#pragma unroll
            for (int c = 0; c < KC; ++c)
                if (c < a.k) {
                    if (update) row_store(a.lam[c], row, l_out[c]);
                    row_store(a.v[c], row, v_out[c]);
                }
        }
        q = qn;
        sub = subn;
    }
    if (!update) return;
    __shared__ double smem[KC * SM_THREADS / 64];
    rbl::block_sum<KC, SM_THREADS>(s_prim, smem);
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (c < a.k) a.partials[c][blockIdx.x * 3] = s_prim[c];
    }
}

// red_k[0] = sum of the blocks' shares of sum (z_k - v_k)^2, red_k[1] = 0 (the loss sum is a pass of its own) - the sum
// order of k_finish_v (sweep_erm.hip); one block per column
struct MultiRed {
    const double* partials[RBL_MULTI_KMAX];
    double* red[RBL_MULTI_KMAX];
};
__global__ __launch_bounds__(256) void k_finish_vm(MultiRed a, int nb) {
    __shared__ double smem[4];
    const double* __restrict__ partials = a.partials[blockIdx.x];
    double s[1] = {0.0};
    for (int b = threadIdx.x; b < nb; b += 256) s[0] += partials[b * 3];
    rbl::block_sum<1, 256>(s, smem);
    if (threadIdx.x == 0) {
        a.red[blockIdx.x][0] = s[0];
        a.red[blockIdx.x][1] = 0.0;
    }
}

// ---- Q pass ------------------------------------------------------------------------------------------------------
// slab: KC planes of (gridDim.x + SM_SLICES) rows of ld doubles; plane c, row b = block b's column sums of column c
template <typename T, int P, int R, int S, int KC>
__global__ __launch_bounds__(SM_THREADS, 1) void k_sweep_qm(const T* __restrict__ D, long long n, long long ld, MultiQ a,
                                                              double* __restrict__ slab, long long plane) {
    constexpr int E = Pk<T>::E;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int PK = (int)(ld / E);
    const unsigned row_bytes = (unsigned)ld * (unsigned)sizeof(T);

    double acc[KC][P][E];
    int boff[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int pkp = lane + 64 * p;
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int k = 0; k < E; ++k) acc[c][p][k] = 0.0;
        boff[p] = pkp < PK ? pkp * 16 : 0x7ffffff0;
    }

    constexpr int SR = S * R;
    const int nsuper = (int)((n + SR - 1) / SR);
    const int live_last = (int)(n - (long long)(nsuper - 1) * SR);
    const int gw = (int)blockIdx.x * (SM_THREADS / 64) + wave;
    const int GW = (int)gridDim.x * (SM_THREADS / 64);

    auto load_side = [&](int q, double (&co)[KC]) {
        const int live = q == nsuper - 1 ? live_last : SR;
        const bool mine = lane < live;
        const long long myrow = (long long)q * SR + lane;
#pragma unroll
        for (int c = 0; c < KC; ++c) co[c] = mine ? a.c[c][myrow] : 0.0;
    };
    auto load_rows = [&](int q, int sub, u32x4 (&buf)[R][P]) {
        const int live = q == nsuper - 1 ? live_last : SR;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int i = sub * R + r;
            if (i >= live) i = live - 1;   // rows past n re-read the last row; their coefficient is 0
            const long long row = (long long)q * SR + i;
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(D + row * ld), 0, (int)row_bytes, 0x00020000);
#pragma unroll
            for (int p = 0; p < P; ++p) buf[r][p] = __builtin_amdgcn_raw_buffer_load_b128(rs, boff[p], 0, RBL_D_AUX);
        }
    };
    auto process = [&](int live, int sub, u32x4 (&buf)[R][P], const double (&co)[KC]) {
        const bool owner = lane >= sub * R && lane < sub * R + R && lane < live;
        double cc[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) cc[c] = owner ? co[c] : 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double cr[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) cr[c] = rbl::readlane_d(cc[c], sub * R + r);
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const double x = Pk<T>::at(buf[r][p], k);
#pragma unroll
                    for (int c = 0; c < KC; ++c) acc[c][p][k] = __builtin_fma(x, cr[c], acc[c][p][k]);
                }
        }
    };

    u32x4 bufA[R][P], bufB[R][P];
    double co[KC], coN[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) co[c] = coN[c] = 0.0;
    int q = gw, sub = 0;
    if (q < nsuper) {
        load_side(q, coN);
        load_rows(q, 0, bufB);
    }
#pragma clang loop unroll(disable)
    while (q < nsuper) {
        const int live = q == nsuper - 1 ? live_last : SR;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int p = 0; p < P; ++p) bufA[r][p] = bufB[r][p];
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < KC; ++c) co[c] = coN[c];
        }
        const bool last = sub + 1 == S;
        const int qn = last ? q + GW : q;
        const int subn = last ? 0 : sub + 1;
        __builtin_amdgcn_sched_barrier(0);
        if (qn < nsuper) {
            if (last) load_side(qn, coN);
            load_rows(qn, subn, bufB);
        }
        __builtin_amdgcn_sched_barrier(0);
        process(live, sub, bufA, co);
        q = qn;
        sub = subn;
    }

    // fold the 4 waves' column sums in LDS (wave order), one slab row per block and column
    __shared__ double red[SM_THREADS / 64][64 * P * E];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int k = 0; k < E; ++k) red[wave][(p * 64 + lane) * E + k] = acc[c][p][k];
        __syncthreads();
        for (int i = tid; i < 64 * P * E; i += SM_THREADS) {
            if (i < ld) {
                double s = 0.0;
#pragma unroll
                for (int wv = 0; wv < SM_THREADS / 64; ++wv) s += red[wv][i];
                slab[(long long)c * plane + (long long)blockIdx.x * ld + i] = s;
            }
        }
        __syncthreads();
    }
}

// the two-stage column reduction of sweep_erm.hip (k_colreduce2 / k_finish_q), one plane per blockIdx.z / .y
__global__ __launch_bounds__(256) void k_colreduce_m(double* __restrict__ slab, long long plane, int nb, long long ld) {
    __shared__ double red[4][64];
    const double* __restrict__ sl = slab + (long long)blockIdx.z * plane;
    double* __restrict__ part = slab + (long long)blockIdx.z * plane + (long long)nb * ld;
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long col = (long long)blockIdx.x * 64 + cx;
    const int slice = blockIdx.y;
    const int per = (nb + SM_SLICES - 1) / SM_SLICES;
    const int b0 = slice * per, b1 = min(nb, b0 + per);
    double acc = 0.0;
    if (col < ld)
        for (int b = b0 + g; b < b1; b += 4) acc += sl[(long long)b * ld + col];
    red[g][cx] = acc;
    __syncthreads();
    if (g == 0 && col < ld) part[(long long)slice * ld + col] = (red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx]);
}
__global__ __launch_bounds__(256) void k_finish_qm(const double* __restrict__ slab, long long plane, int nb, long long ld,
                                                    MultiQ a) {
    const double* __restrict__ part = slab + (long long)blockIdx.y * plane + (long long)nb * ld;
    double* __restrict__ q = a.q[blockIdx.y];
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < ld; j += (long long)gridDim.x * 256) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < SM_SLICES; ++k) s += part[(long long)k * ld + j];
        q[j] = s;
    }
}

// shapes (P, R, S) of launch_v_T / launch_q_T (sweep_erm.hip); every multi-column kernel runs one block per CU
template <typename T, int KC>
int launch_vm_T(const T* D, long long n, long long ld, const MultiV& a, int grid, SweepInstance* inst, hipStream_t s) {
    const long long passes = (ld / Pk<T>::E + 63) / 64;
#define RBL_VM(P_, R_, S_)                                                                                               \
    do {                                                                                                                 \
        auto kfn = k_sweep_vm<T, P_, R_, S_, KC>;                                                                        \
        const size_t lds = (size_t)KC * 64 * P_ * Pk<T>::E * sizeof(double);                                             \
        static bool attr_set = false;                                                                                    \
        if (!attr_set && lds > 32768) {                                                                                  \
            RBL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                        (int)lds));                                                                      \
            attr_set = true;                                                                                             \
        }                                                                                                                \
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(SM_THREADS), lds, s, D, n, ld, a);                                      \
        RBL_HIP(hipGetLastError());                                                                                      \
        sweep_report(inst, SWEEP_KIND_WAVE, P_, R_, S_, grid);                                                           \
        return RBL_OK;                                                                                                   \
    } while (0)
    if (passes == 1) RBL_VM(1, 8, 2);
    if (passes == 2) RBL_VM(2, 4, 4);
    if (passes <= 4) RBL_VM(4, 2, 8);
    if constexpr (sizeof(T) > 2) {   // fp16 storage: up to 4 packets per lane (sweep_multi_supported)
        if (passes <= 8) RBL_VM(8, 2, 8);
    }
#undef RBL_VM
    rbl_set_error("multi-column V pass: ld=%lld outside the wave-per-row range", ld);
    return RBL_ERR_INVALID;
}

template <typename T, int KC>
int launch_qm_T(const T* D, long long n, long long ld, const MultiQ& a, double* slab, long long plane, int grid, SweepInstance* inst,
                hipStream_t s) {
    const long long passes = (ld / Pk<T>::E + 63) / 64;
#define RBL_QM(P_, R_, S_)                                                                                              \
    do {                                                                                                                \
        hipLaunchKernelGGL((k_sweep_qm<T, P_, R_, S_, KC>), dim3(grid), dim3(SM_THREADS), 0, s, D, n, ld, a, slab, plane); \
        RBL_HIP(hipGetLastError());                                                                                     \
        sweep_report(inst, SWEEP_KIND_WAVE, P_, R_, S_, grid);                                                          \
        return RBL_OK;                                                                                                  \
    } while (0)
    if (passes == 1) RBL_QM(1, 8, 2);
    if (passes == 2) RBL_QM(2, 4, 4);
    if (passes <= 4) RBL_QM(4, 2, 8);
    if constexpr (sizeof(T) > 2) {
        if (passes <= 8) RBL_QM(8, 2, 8);
    }
#undef RBL_QM
    rbl_set_error("multi-column Q pass: ld=%lld outside the wave-per-row range", ld);
    return RBL_ERR_INVALID;
}

}  // namespace

// fp16 storage: the Q pass keeps K x P x 8 fp64 column sums per lane - 4 packets per lane (ld <= 2048) are the 256
// registers that 8 packets are with fp32 storage, so the shared range ends at the same width in ELEMENTS and begins, as
// everywhere, above 32 packets per row (ld > 256); wider fp16 rows run each member's own passes
bool sweep_multi_supported(int storage, int64_t ld) {
    if (storage == RBL_STORE_CSR) return false;   // no shared multi-column sparse passes: every member runs its own
    if (storage == RBL_STORE_F16) return sweep_v_supported(storage, ld) && ld <= 2048;
    return sweep_v_supported(storage, ld);
}

// columns one launch carries: 4 for every supported width and every storage type (the Q pass' column sums at 8 packets
// per lane and fp32 storage are 256 of the 512 registers a lane of the one block per CU may use; 8 columns do not fit)
int sweep_multi_k(int storage, int64_t ld) {
    (void)storage;
    (void)ld;
    return RBL_MULTI_KMAX;
}

size_t sweep_multi_slab_doubles(int64_t ld, int num_cu) { return (size_t)RBL_MULTI_KMAX * (size_t)(num_cu + SM_SLICES) * (size_t)ld; }

int launch_sweep_v_multi(int storage, const void* D, int64_t n, int64_t ld, int k, const double* const* w, const double* const* z,
                         double* const* lam, double* const* v, const double* rho, double* const* partials, double* const* red,
                         int num_cu, hipStream_t s, SweepInstance* inst) {
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("multi-column V pass: %d columns in one launch (1..%d)", k, RBL_MULTI_KMAX);
        return RBL_ERR_INVALID;
    }
    if (n <= 0) return RBL_OK;
    const bool update = z != nullptr;
    MultiV a;
    MultiRed r;
    for (int c = 0; c < RBL_MULTI_KMAX; ++c) {
        const int j = c < k ? c : 0;
        a.w[c] = w[j];
        a.v[c] = v[j];
        a.z[c] = update ? z[j] : nullptr;
        a.lam[c] = update ? lam[j] : nullptr;
        a.partials[c] = update ? partials[j] : nullptr;
        a.rho[c] = update ? rho[j] : 0.0;
        r.partials[c] = a.partials[c];
        r.red[c] = update ? red[j] : nullptr;
    }
    a.k = k;
    a.update = update ? 1 : 0;
    const int grid = num_cu;
    int rc;
    if (storage == RBL_STORE_F32)
        rc = k <= 2 ? launch_vm_T<float, 2>((const float*)D, n, ld, a, grid, inst, s) : launch_vm_T<float, 4>((const float*)D, n, ld, a, grid, inst, s);
    else if (storage == RBL_STORE_F16)
        rc = k <= 2 ? launch_vm_T<rbl_half, 2>((const rbl_half*)D, n, ld, a, grid, inst, s) : launch_vm_T<rbl_half, 4>((const rbl_half*)D, n, ld, a, grid, inst, s);
    else
        rc = k <= 2 ? launch_vm_T<double, 2>((const double*)D, n, ld, a, grid, inst, s) : launch_vm_T<double, 4>((const double*)D, n, ld, a, grid, inst, s);
    RBL_TRY(rc);
    if (update) {
        hipLaunchKernelGGL(k_finish_vm, dim3(k), dim3(256), 0, s, r, grid);
        RBL_HIP(hipGetLastError());
    }
    return RBL_OK;
}

int launch_sweep_q_multi(int storage, const void* D, int64_t n, int64_t ld, int k, const double* const* c, double* slab,
                         double* const* q, int num_cu, hipStream_t s, SweepInstance* inst) {
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("multi-column Q pass: %d columns in one launch (1..%d)", k, RBL_MULTI_KMAX);
        return RBL_ERR_INVALID;
    }
    if (n <= 0) {
        for (int j = 0; j < k; ++j) RBL_HIP(hipMemsetAsync(q[j], 0, sizeof(double) * ld, s));
        return RBL_OK;
    }
    MultiQ a;
    for (int j = 0; j < RBL_MULTI_KMAX; ++j) {
        a.c[j] = c[j < k ? j : 0];
        a.q[j] = q[j < k ? j : 0];
    }
    a.k = k;
    const int grid = num_cu;
    const long long plane = (long long)(grid + SM_SLICES) * ld;
    int rc;
    if (storage == RBL_STORE_F32)
        rc = k <= 2 ? launch_qm_T<float, 2>((const float*)D, n, ld, a, slab, plane, grid, inst, s)
                    : launch_qm_T<float, 4>((const float*)D, n, ld, a, slab, plane, grid, inst, s);
    else if (storage == RBL_STORE_F16)
        rc = k <= 2 ? launch_qm_T<rbl_half, 2>((const rbl_half*)D, n, ld, a, slab, plane, grid, inst, s)
                    : launch_qm_T<rbl_half, 4>((const rbl_half*)D, n, ld, a, slab, plane, grid, inst, s);
    else
        rc = k <= 2 ? launch_qm_T<double, 2>((const double*)D, n, ld, a, slab, plane, grid, inst, s)
                    : launch_qm_T<double, 4>((const double*)D, n, ld, a, slab, plane, grid, inst, s);
    RBL_TRY(rc);
    hipLaunchKernelGGL(k_colreduce_m, dim3((unsigned)((ld + 63) / 64), SM_SLICES, (unsigned)k), dim3(256), 0, s, slab, plane, grid,
                       (long long)ld);
    hipLaunchKernelGGL(k_finish_qm, dim3((unsigned)((ld + 255) / 256), (unsigned)k), dim3(256), 0, s, (const double*)slab, plane,
                       grid, (long long)ld, a);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}
