// sweep.hip - the two HBM-bound streaming passes over the n x d matrix D = -y*X that
// every ADMM iteration needs:
//   v = D w      replaces the three GEMVs of src/optim/algorithms.py:89,132,135
//   q = D^T c    replaces the n-space sweeps of src/util/fast_lasso.py:41,43,55 and
//                src/util/w_LBFGS.py:34,43 (the w-step then runs in d-space on G = D^T D)
// D is row-major, ld % 4 == 0, stored fp32 (default), fp64 or fp16 (ld % 8 == 0); accumulation is fp64.
// Both kernels read D exactly once with 16-byte per-lane loads (1 KiB per wave
// instruction); they are memory bound: algorithmic bytes = n*ld*sizeof(T) per launch.
#include "rbl_internal.h"
#include "device_math.h"

namespace {

template <typename T> struct Pkt;  // one 16-byte packet
template <> struct Pkt<float> {
    static constexpr int E = 4;
    typedef float4 type;
    __device__ static inline void fma(const float4& p, const double* w, double& acc) {
        acc = __builtin_fma((double)p.x, w[0], acc);
        acc = __builtin_fma((double)p.y, w[1], acc);
        acc = __builtin_fma((double)p.z, w[2], acc);
        acc = __builtin_fma((double)p.w, w[3], acc);
    }
    __device__ static inline void axpy(const float4& p, double c, double* acc) {
        acc[0] = __builtin_fma((double)p.x, c, acc[0]);
        acc[1] = __builtin_fma((double)p.y, c, acc[1]);
        acc[2] = __builtin_fma((double)p.z, c, acc[2]);
        acc[3] = __builtin_fma((double)p.w, c, acc[3]);
    }
};
template <> struct Pkt<double> {
    static constexpr int E = 2;
    typedef double2 type;
    __device__ static inline void fma(const double2& p, const double* w, double& acc) {
        acc = __builtin_fma(p.x, w[0], acc);
        acc = __builtin_fma(p.y, w[1], acc);
    }
    __device__ static inline void axpy(const double2& p, double c, double* acc) {
        acc[0] = __builtin_fma(p.x, c, acc[0]);
        acc[1] = __builtin_fma(p.y, c, acc[1]);
    }
};

// fp16 storage: 8 halves per packet, element k = the low (k even) or high half of dword k / 2, widened
// half -> float -> double (both exact)
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <> struct Pkt<rbl_half> {
    static constexpr int E = 8;
    typedef u32x4_t type;
    __device__ static inline double at(const u32x4_t& p, int k) {
        const unsigned short h = (unsigned short)((k & 1) ? p[k >> 1] >> 16 : p[k >> 1]);
        return (double)(float)__builtin_bit_cast(_Float16, h);
    }
    __device__ static inline void fma(const u32x4_t& p, const double* w, double& acc) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = __builtin_fma(at(p, k), w[k], acc);
    }
    __device__ static inline void axpy(const u32x4_t& p, double c, double* acc) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = __builtin_fma(at(p, k), c, acc[k]);
    }
};

// D is streamed once per pass and is far larger than L2 + MALL: the loads carry the non-temporal hint (measured on
// MI355X: +8 % on the single-sweep kernel; RBL_D_STREAM=0 at compile time restores plain loads)
#ifndef RBL_D_STREAM
#define RBL_D_STREAM 1
#endif
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));
__device__ inline float4 ld_stream(const float4* p) {
#if RBL_D_STREAM
    const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ inline double2 ld_stream(const double2* p) {
#if RBL_D_STREAM
    const f64x2_t v = __builtin_nontemporal_load(reinterpret_cast<const f64x2_t*>(p));
    return make_double2(v.x, v.y);
#else
    return *p;
#endif
}

__device__ inline u32x4_t ld_stream(const u32x4_t* p) {
#if RBL_D_STREAM
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

__device__ inline double shfl_xor_d(double x, int mask) {
    return __shfl_xor(x, mask, 64);
}

// ------------------------------------------------------------------------------ v = D w
// LPR lanes share one row (power of two <= 64); a wave covers 64/LPR rows per pass and
// keeps U row-groups in flight.  P = passes of LPR packets per row, compile-time so the
// U*P loads of a step are issued back to back and w lives in registers; P == 0 selects
// the generic path (w staged in LDS, run-time pass loop) for large d.
template <typename T, int LPR, int P, int U>
__global__ __launch_bounds__(256) void k_gemv(const T* __restrict__ D, long long n, long long ld,
                                                 const double* __restrict__ w, double* __restrict__ v) {
    typedef typename Pkt<T>::type pkt_t;
    constexpr int E = Pkt<T>::E;
    constexpr int RPW = 64 / LPR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % LPR, rsub = lane / LPR;
    const long long PK = ld / E;
    const long long rows_per_step = (long long)RPW * U;
    const long long stride = (long long)gridDim.x * 4 * rows_per_step;

    double wr[P > 0 ? P : 1][E];
    extern __shared__ double sw[];
    if (P > 0) {
#pragma unroll
        for (int p = 0; p < (P > 0 ? P : 1); ++p) {
            long long pk = sub + (long long)p * LPR;
#pragma unroll
            for (int k = 0; k < E; ++k) wr[p][k] = (pk < PK) ? w[pk * E + k] : 0.0;
        }
    } else {
        for (long long i = tid; i < ld; i += 256) sw[i] = w[i];
        __syncthreads();
    }

    for (long long rbase = ((long long)blockIdx.x * 4 + wave) * rows_per_step; rbase < n; rbase += stride) {
        double acc[U];
        const pkt_t* rowp[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = rbase + (long long)u * RPW + rsub;
            if (r >= n) r = n - 1;  // clamp: read a valid row, result discarded below
            rowp[u] = reinterpret_cast<const pkt_t*>(D + r * ld);
            acc[u] = 0.0;
        }
        if (P > 0) {
            pkt_t buf[U][P > 0 ? P : 1];
#pragma unroll
            for (int p = 0; p < (P > 0 ? P : 1); ++p) {
                long long pk = sub + (long long)p * LPR;
                if (pk >= PK) pk = PK - 1;  // tail lanes re-read the last packet with w == 0
#pragma unroll
                for (int u = 0; u < U; ++u) buf[u][p] = ld_stream(rowp[u] + pk);
            }
#pragma unroll
            for (int p = 0; p < (P > 0 ? P : 1); ++p)
#pragma unroll
                for (int u = 0; u < U; ++u) Pkt<T>::fma(buf[u][p], wr[p], acc[u]);
        } else {
            // large d: w lives in LDS; 4 passes x U rows = 16 loads are issued before they are
            // consumed so that enough bytes stay in flight at the low occupancy LDS leaves
            constexpr int PB = 4;
            long long pk = sub;
            for (; pk + (long long)(PB - 1) * LPR < PK; pk += (long long)PB * LPR) {
                pkt_t x[PB][U];
#pragma unroll
                for (int b = 0; b < PB; ++b)
#pragma unroll
                    for (int u = 0; u < U; ++u) x[b][u] = ld_stream(rowp[u] + pk + (long long)b * LPR);
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    const double* wp = sw + (pk + (long long)b * LPR) * E;
#pragma unroll
                    for (int u = 0; u < U; ++u) Pkt<T>::fma(x[b][u], wp, acc[u]);
                }
            }
            for (; pk < PK; pk += LPR) {
                const double* wp = sw + pk * E;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    pkt_t x = ld_stream(rowp[u] + pk);
                    Pkt<T>::fma(x, wp, acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (LPR == 64) {
                acc[u] = rbl::wave_sum_all(acc[u]);  // DPP butterfly + readlanes (device_math.h)
            } else {
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) acc[u] += shfl_xor_d(acc[u], off);
            }
            long long r = rbase + (long long)u * RPW + rsub;
            if (sub == 0 && r < n) v[r] = acc[u];
        }
    }
}

template <typename T, int LPR>
int gemv_dispatch(const T* D, long long n, long long ld, const double* w, double* v, int num_cu, hipStream_t s,
                  PassInstance* inst) {
    constexpr int E = Pkt<T>::E;
    const long long PK = ld / E;
    const long long passes = (PK + LPR - 1) / LPR;
    int grid = num_cu * 8;
    const long long rows_per_block = 4LL * (64 / LPR) * 2;
    long long need = (n + rows_per_block - 1) / rows_per_block;
    if (need < grid) grid = (int)(need > 0 ? need : 1);
    if constexpr (LPR < 64) {
        // a row fits one pass of its lane group
        hipLaunchKernelGGL((k_gemv<T, LPR, 1, 4>), dim3(grid), dim3(256), 0, s, D, n, ld, w, v);
        pass_report(inst, PASS_ROUTE_PLAIN, LPR, 1, 4, grid, 1);
    } else {
        if (passes == 1) {
            hipLaunchKernelGGL((k_gemv<T, LPR, 1, 4>), dim3(grid), dim3(256), 0, s, D, n, ld, w, v);
            pass_report(inst, PASS_ROUTE_PLAIN, LPR, 1, 4, grid, 1);
        } else if (passes == 2) {
            hipLaunchKernelGGL((k_gemv<T, LPR, 2, 4>), dim3(grid), dim3(256), 0, s, D, n, ld, w, v);
            pass_report(inst, PASS_ROUTE_PLAIN, LPR, 2, 4, grid, 1);
        } else if (passes <= 4) {
            hipLaunchKernelGGL((k_gemv<T, LPR, 4, 2>), dim3(grid), dim3(256), 0, s, D, n, ld, w, v);
            pass_report(inst, PASS_ROUTE_PLAIN, LPR, 4, 2, grid, 1);
        } else if (passes <= 8) {
            hipLaunchKernelGGL((k_gemv<T, LPR, 8, 1>), dim3(grid), dim3(256), 0, s, D, n, ld, w, v);
            pass_report(inst, PASS_ROUTE_PLAIN, LPR, 8, 1, grid, 1);
        } else {
            size_t lds = (size_t)ld * sizeof(double);
            if (lds > 150 * 1024) {
                rbl_set_error("gemv: d too large for the LDS-staged path (ld=%lld)", ld);
                return RBL_ERR_INVALID;
            }
            if (lds > 64 * 1024) {
                RBL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemv<T, LPR, 0, 4>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
            hipLaunchKernelGGL((k_gemv<T, LPR, 0, 4>), dim3(grid), dim3(256), lds, s, D, n, ld, w, v);
            pass_report(inst, PASS_ROUTE_PLAIN, LPR, 0, 4, grid, 1);
        }
    }
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

template <typename T>
int gemv_T(const T* D, long long n, long long ld, const double* w, double* v, int num_cu, hipStream_t s, PassInstance* inst) {
    const long long PK = ld / Pkt<T>::E;
    if (PK > 32) return gemv_dispatch<T, 64>(D, n, ld, w, v, num_cu, s, inst);
    if (PK > 16) return gemv_dispatch<T, 32>(D, n, ld, w, v, num_cu, s, inst);
    if (PK > 8) return gemv_dispatch<T, 16>(D, n, ld, w, v, num_cu, s, inst);
    if (PK > 4) return gemv_dispatch<T, 8>(D, n, ld, w, v, num_cu, s, inst);
    if (PK > 2) return gemv_dispatch<T, 4>(D, n, ld, w, v, num_cu, s, inst);
    if (PK > 1) return gemv_dispatch<T, 2>(D, n, ld, w, v, num_cu, s, inst);
    return gemv_dispatch<T, 1>(D, n, ld, w, v, num_cu, s, inst);
}

// ---------------------------------------------------------------------------- q = D^T c
// TPR threads share one row (power of two <= 256); the block covers 256/TPR rows per
// step with U steps in flight; thread `sub` owns packets sub + j*TPR (j < PJ) of the
// column tile blockIdx.y, so partial column sums stay in registers for the block's
// whole row range.  One slab row per block, reduced by k_colreduce (deterministic).
// SQ = true accumulates c*x^2 as well (column statistics).
template <typename T, int TPR, int PJ, int U, bool SQ>
__global__ __launch_bounds__(256) void k_gemvt(const T* __restrict__ D, long long n, long long ld,
                                                  const double* __restrict__ c, double* __restrict__ slab,
                                                  double* __restrict__ slab2) {
    typedef typename Pkt<T>::type pkt_t;
    constexpr int E = Pkt<T>::E;
    constexpr int RPB = 256 / TPR;
    const int tid = threadIdx.x;
    const int sub = tid % TPR, rsub = tid / TPR;
    const long long PK = ld / E;
    const long long col0 = (long long)blockIdx.y * TPR * PJ;  // first packet of this column tile
    // contiguous row range of this block
    const long long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
    const long long r_begin = (long long)blockIdx.x * rows_per_block;
    long long r_end = r_begin + rows_per_block;
    if (r_end > n) r_end = n;

    double acc[PJ][E];
    double acc2[SQ ? PJ : 1][E];
#pragma unroll
    for (int j = 0; j < PJ; ++j)
#pragma unroll
        for (int k = 0; k < E; ++k) {
            acc[j][k] = 0.0;
            if (SQ) acc2[j][k] = 0.0;
        }
    long long pk[PJ];
    bool pkv[PJ];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        pk[j] = col0 + sub + (long long)j * TPR;
        pkv[j] = pk[j] < PK;
        if (!pkv[j]) pk[j] = PK - 1;
    }

    for (long long rbase = r_begin; rbase < r_end; rbase += (long long)RPB * U) {
        pkt_t buf[U][PJ];
        double cv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = rbase + (long long)u * RPB + rsub;
            bool ok = r < r_end;
            if (!ok) r = r_end - 1;
            cv[u] = ok ? (c ? c[r] : 1.0) : 0.0;
            const pkt_t* rp = reinterpret_cast<const pkt_t*>(D + r * ld);
#pragma unroll
            for (int j = 0; j < PJ; ++j) buf[u][j] = ld_stream(rp + pk[j]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < PJ; ++j) Pkt<T>::axpy(buf[u][j], cv[u], acc[j]);
        if (SQ) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < PJ; ++j) {
                    if constexpr (E == 4) {
                        double a = (double)buf[u][j].x, b = (double)buf[u][j].y, cc = (double)buf[u][j].z,
                               dd = (double)buf[u][j].w;
                        acc2[j][0] = __builtin_fma(a * a, cv[u], acc2[j][0]);
                        acc2[j][1] = __builtin_fma(b * b, cv[u], acc2[j][1]);
                        acc2[j][2] = __builtin_fma(cc * cc, cv[u], acc2[j][2]);
                        acc2[j][3] = __builtin_fma(dd * dd, cv[u], acc2[j][3]);
                    } else {
                        double a = (double)buf[u][j].x, b = (double)buf[u][j].y;
                        acc2[j][0] = __builtin_fma(a * a, cv[u], acc2[j][0]);
                        acc2[j][1] = __builtin_fma(b * b, cv[u], acc2[j][1]);
                    }
                }
        }
    }

    // fold the RPB row groups of the block (only when a row is narrower than the block)
    if (RPB > 1) {
        __shared__ double red[256 * (E > 4 ? E : 4)];
        for (int pass = 0; pass < (SQ ? 2 : 1); ++pass) {
#pragma unroll
            for (int j = 0; j < PJ; ++j) {
                __syncthreads();
#pragma unroll
                for (int k = 0; k < E; ++k) red[tid * E + k] = pass ? acc2[SQ ? j : 0][k] : acc[j][k];
                __syncthreads();
                if (rsub == 0) {
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                        double sacc = 0.0;
                        for (int g = 0; g < RPB; ++g) sacc += red[(g * TPR + sub) * E + k];
                        if (pass) acc2[SQ ? j : 0][k] = sacc; else acc[j][k] = sacc;
                    }
                }
            }
        }
    }
    if (rsub == 0) {
#pragma unroll
        for (int j = 0; j < PJ; ++j)
            if (pkv[j]) {
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    slab[(long long)blockIdx.x * ld + pk[j] * E + k] = acc[j][k];
                    if (SQ) slab2[(long long)blockIdx.x * ld + pk[j] * E + k] = acc2[j][k];
                }
            }
    }
}

// q[j] = sum_b slab[b][j]: 64 columns x 16 row groups per block, fixed summation order.
__global__ __launch_bounds__(1024) void k_colreduce(const double* __restrict__ slab, int nb, long long ld,
                                                      double* __restrict__ q) {
    __shared__ double red[16][64];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long col = (long long)blockIdx.x * 64 + cx;
    double acc = 0.0;
    if (col < ld)
        for (int b = g; b < nb; b += 16) acc += slab[(long long)b * ld + col];
    red[g][cx] = acc;
    __syncthreads();
    if (g == 0 && col < ld) {
        double sacc = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) sacc += red[k][cx];
        q[col] = sacc;
    }
}

#ifndef RBL_GEMVT_BPC
#define RBL_GEMVT_BPC 4
#endif
#ifndef RBL_GEMVT_U
#define RBL_GEMVT_U 8   // rows in flight per thread in the one-packet-per-thread instance (d <= 1024 fp32)
#endif
constexpr int GEMVT_BLOCKS_PER_CU = RBL_GEMVT_BPC;

template <typename T, int TPR, bool SQ>
int gemvt_dispatch(const T* D, long long n, long long ld, const double* c, double* slab, double* slab2,
                   int nblocks, hipStream_t s, PassInstance* inst) {
    constexpr int E = Pkt<T>::E;
    const long long PK = ld / E;
    long long pj = (PK + TPR - 1) / TPR;
    int ytiles = 1;
    if (pj > 8) {
        ytiles = (int)((pj + 7) / 8);
        pj = 8;
    }
    dim3 grid(nblocks, ytiles);
    if constexpr (TPR < 256) {
        hipLaunchKernelGGL((k_gemvt<T, TPR, 1, 8, SQ>), grid, dim3(256), 0, s, D, n, ld, c, slab, slab2);
        pass_report(inst, PASS_ROUTE_PLAIN, TPR, 1, 8, nblocks, ytiles);
    } else {
        if (pj == 1) {
            hipLaunchKernelGGL((k_gemvt<T, TPR, 1, RBL_GEMVT_U, SQ>), grid, dim3(256), 0, s, D, n, ld, c, slab, slab2);
            pass_report(inst, PASS_ROUTE_PLAIN, TPR, 1, RBL_GEMVT_U, nblocks, ytiles);
        } else if (pj == 2) {
            hipLaunchKernelGGL((k_gemvt<T, TPR, 2, 4, SQ>), grid, dim3(256), 0, s, D, n, ld, c, slab, slab2);
            pass_report(inst, PASS_ROUTE_PLAIN, TPR, 2, 4, nblocks, ytiles);
        } else if (pj <= 4) {
            hipLaunchKernelGGL((k_gemvt<T, TPR, 4, 2, SQ>), grid, dim3(256), 0, s, D, n, ld, c, slab, slab2);
            pass_report(inst, PASS_ROUTE_PLAIN, TPR, 4, 2, nblocks, ytiles);
        } else {
            hipLaunchKernelGGL((k_gemvt<T, TPR, 8, 1, SQ>), grid, dim3(256), 0, s, D, n, ld, c, slab, slab2);
            pass_report(inst, PASS_ROUTE_PLAIN, TPR, 8, 1, nblocks, ytiles);
        }
    }
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

template <typename T, bool SQ>
int gemvt_T(const T* D, long long n, long long ld, const double* c, double* slab, double* slab2, int nblocks,
            hipStream_t s, PassInstance* inst) {
    const long long PK = ld / Pkt<T>::E;
    if (PK > 128) return gemvt_dispatch<T, 256, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 64) return gemvt_dispatch<T, 128, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 32) return gemvt_dispatch<T, 64, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 16) return gemvt_dispatch<T, 32, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 8) return gemvt_dispatch<T, 16, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 4) return gemvt_dispatch<T, 8, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 2) return gemvt_dispatch<T, 4, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    if (PK > 1) return gemvt_dispatch<T, 2, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
    return gemvt_dispatch<T, 1, SQ>(D, n, ld, c, slab, slab2, nblocks, s, inst);
}

int gemvt_blocks(int num_cu, long long n) {
    long long nb = (long long)num_cu * GEMVT_BLOCKS_PER_CU;
    long long cap = (n + 63) / 64;  // at least 64 rows per block
    if (cap < 1) cap = 1;
    if (nb > cap) nb = cap;
    return (int)nb;
}

// ------------------------------------------------------------------- forming / reading D
template <typename T>
__global__ void k_D_to_f64(const T* __restrict__ D, long long ld, long long n, long long d,
                           double* __restrict__ out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    long long r = i / d, j = i - r * d;
    out[i] = (double)D[r * ld + j];   // (fp16: half -> float -> double, exact)
}
template <typename T>
__global__ void k_standardize_negy(T* __restrict__ D, long long n, long long ld, long long d,
                                   const double* __restrict__ mean, const double* __restrict__ inv_std,
                                   const signed char* __restrict__ ysign) {
    // grid-stride: n * ld exceeds 2^32 at the full-size configurations (6e9 elements at C2), and a HIP
    // launch of more than 2^32 threads wraps - round 1 launched one thread per element here and left the
    // rows beyond the wrap unstandardised (caught by tests/test_gpu_fullsize.py)
    const long long total = n * ld;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / ld, j = i - r * ld;
        if (j >= d) continue;
        const double x = ((double)D[i] - mean[j]) * inv_std[j];
        D[i] = (T)(-(double)ysign[r] * x);
    }
}

// ------------------------------------------------- typed sources (rbl_set_data_from): X as the caller holds it
// S = double / float / unsigned short (IEEE binary16 bits); widening to double is exact.
__device__ inline double src_widen(double x) { return x; }
__device__ inline double src_widen(float x) { return (double)x; }
__device__ inline double src_widen(unsigned short x) { return (double)(float)__builtin_bit_cast(_Float16, x); }

template <int W> struct SrcDw;   // W dwords loaded at once
template <> struct SrcDw<1> { typedef unsigned int type; };
template <> struct SrcDw<2> { typedef unsigned int type __attribute__((ext_vector_type(2))); };
template <> struct SrcDw<4> { typedef u32x4_t type; };
// bytes one load instruction of the packet-wise path moves for this pair of types: 16, or the E source elements of one
// output packet when those are fewer (half -> f32: 8, half -> f64: 4).  Base and row stride must be multiples of it.
template <typename S, int E> struct SrcLoad {
    static constexpr int BYTES = E * (int)sizeof(S), UNIT = BYTES < 16 ? BYTES : 16, NL = BYTES / UNIT;
};
// the E source elements behind one output packet (read once, non-temporal: X is streamed and far larger than L2 + MALL)
template <typename S, int E>
__device__ inline void src_load_vec(const S* __restrict__ p, double* xs) {
    typedef SrcLoad<S, E> L;
    typedef typename SrcDw<L::UNIT / 4>::type vec_t;
    union {
        vec_t v[L::NL];
        S e[E];
    } u;
#pragma unroll
    for (int l = 0; l < L::NL; ++l) u.v[l] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(p) + l);
#pragma unroll
    for (int k = 0; k < E; ++k) xs[k] = src_widen(u.e[k]);
}

template <typename T> struct StorePkt;   // one 16-byte packet of the padded row, from E fp64 values
template <> struct StorePkt<double> {
    static constexpr int E = 2;
    __device__ static inline void put(double* p, const double* v, u64*, long long) { *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]); }
};
template <> struct StorePkt<float> {
    static constexpr int E = 4;
    __device__ static inline void put(float* p, const double* v, u64*, long long) {
        *reinterpret_cast<float4*>(p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    }
};
template <> struct StorePkt<rbl_half> {
    static constexpr int E = 8;
    // one rounding from the fp64 value; finite in, infinite out: counted, the first one (smallest row * d + column) kept
    __device__ static inline void put(rbl_half* p, const double* v, u64* ovf, long long pos0) {
        u32x4_t w;
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const unsigned short lo = f64_to_f16_bits(v[k]), hi = f64_to_f16_bits(v[k + 1]);
            if (f16_bits_inf(lo) && v[k] - v[k] == 0.0) {
                atomicAdd(&ovf[0], 1ull);
                atomicMin(&ovf[1], (u64)(pos0 + k));
            }
            if (f16_bits_inf(hi) && v[k + 1] - v[k + 1] == 0.0) {
                atomicAdd(&ovf[0], 1ull);
                atomicMin(&ovf[1], (u64)(pos0 + k + 1));
            }
            w[k >> 1] = (unsigned)lo | ((unsigned)hi << 16);
        }
        *reinterpret_cast<u32x4_t*>(p) = w;
    }
};

// D[row0 + r][j] = round_to_storage(-y_r * x)  with x = widen(X[r][j]) (SC = false) or (widen(X[r][j]) - mean[j]) * inv[j]
// (SC = true, the arithmetic of k_standardize_negy formed straight from the source: one rounding).  Columns ds <= j < d
// (the column of ones, ds = d - 1) are -y_r * 1, columns >= d the zero pad.  1 << tpr_log threads share a row, a thread
// owns whole 16-byte packets of the padded row and reads the row's sign once; rows are taken in a grid-stride loop and
// every index is 64-bit (n * ld exceeds 2^32 at the project's sizes).  VEC: the source packets are read with
// SrcLoad::UNIT-byte loads (base and row stride allow it); a packet that reaches beyond column ds, and every packet
// when VEC is false (d = 1001 in fp32, a sliced tensor), is read element by element.
template <typename S, typename T, bool SC, bool VEC>
__global__ __launch_bounds__(256) void k_form_src(T* __restrict__ D, long long ld, long long row0, const S* __restrict__ X,
                                                   long long ldx, const signed char* __restrict__ ysign, long long rows,
                                                   long long ds, long long d, const double* __restrict__ mean,
                                                   const double* __restrict__ inv, int tpr_log, u64* ovf) {
    constexpr int E = StorePkt<T>::E;
    const int tpr = 1 << tpr_log, sub = (int)threadIdx.x & (tpr - 1), rsub = (int)threadIdx.x >> tpr_log;
    const long long rpb = 256 >> tpr_log, PK = ld / E;
    // U rows per thread and step: their loads are issued together, the packet's means / inverse scales are read once for
    // the U rows, then the rows are converted and stored (profiles/upload_sources.json: against one row per step, "*_one_row"
    // there, 14.5 -> 11.4 ms with scaling and 11.0 -> 10.8 ms without at 6 000 000 x 1000 fp32)
    constexpr int U = E == 8 ? 2 : 4;
    const long long rstep = (long long)gridDim.x * rpb;
    for (long long rb = (long long)blockIdx.x * rpb + rsub; rb < rows; rb += rstep * U) {
        double ny[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = rb + u * rstep;
            ny[u] = r < rows ? -(double)ysign[r] : 0.0;
        }
        for (long long k = sub; k < PK; k += tpr) {
            const long long j0 = k * E;
            double v[U][E];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long r = rb + u * rstep;
                if (r >= rows) continue;
                const S* __restrict__ xr = X + r * ldx;
                if (VEC && j0 + E <= ds) {
                    src_load_vec<S, E>(xr + j0, v[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) v[u][e] = (j0 + e < ds) ? src_widen(xr[j0 + e]) : 0.0;
                }
            }
            double mj[SC ? E : 1], ij[SC ? E : 1];   // the packet's means and inverse scales, once for the U rows
            if (SC) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    mj[e] = (j0 + e < ds) ? mean[j0 + e] : 0.0;
                    ij[e] = (j0 + e < ds) ? inv[j0 + e] : 1.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long r = rb + u * rstep;
                if (r >= rows) continue;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const long long j = j0 + e;
                    if (j < ds) {
                        double x = v[u][e];
                        if (SC) x = (x - mj[e]) * ij[e];
                        v[u][e] = ny[u] * x;
                    } else {
                        v[u][e] = (j < d) ? ny[u] * 1.0 : 0.0;
                    }
                }
                // (fp16 storage: the pad and the ones never overflow, so pos0 + e only ever names a column < d)
                StorePkt<T>::put(D + (row0 + r) * ld + j0, v[u], ovf, (row0 + r) * d + j0);
            }
        }
    }
}

// Shifted column sums of a typed source, in an order fixed by the row count alone: rows are cut into blocks of
// SRC_STAT_ROWS; one thread per (block, column) adds s1 += x - shift, s2 += (x - shift)^2 in row order; the blocks' sums
// go to slab rows blk0 + b and are folded by k_colreduce (a fixed tree over the block index).  Neither the grid nor the
// chunks a host source arrives in (whole row blocks) change a bit of the result.
constexpr int SRC_STAT_ROWS = 1024;
template <typename S>
__global__ __launch_bounds__(256) void k_src_colstats(const S* __restrict__ X, long long ldx, long long rows, long long ds,
                                                       const double* __restrict__ shift, double* __restrict__ slab1,
                                                       double* __restrict__ slab2, long long ld, long long blk0) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= ds) return;
    const double c = shift[j];
    const long long nb = (rows + SRC_STAT_ROWS - 1) / SRC_STAT_ROWS;
    for (long long b = blockIdx.y; b < nb; b += gridDim.y) {
        const long long r0 = b * SRC_STAT_ROWS;
        const long long r1 = r0 + SRC_STAT_ROWS < rows ? r0 + SRC_STAT_ROWS : rows;
        double s1 = 0.0, s2 = 0.0;
        long long r = r0;
        for (; r + 8 <= r1; r += 8) {   // eight loads in flight, added in row order
            S x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = __builtin_nontemporal_load(X + (r + u) * ldx + j);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double dl = src_widen(x[u]) - c;
                s1 += dl;
                s2 += dl * dl;
            }
        }
        for (; r < r1; ++r) {
            const double dl = src_widen(X[r * ldx + j]) - c;
            s1 += dl;
            s2 += dl * dl;
        }
        slab1[(blk0 + b) * ld + j] = s1;
        slab2[(blk0 + b) * ld + j] = s2;
    }
}
template <typename S>
__global__ void k_src_row(const S* __restrict__ X, long long ds, double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ds) out[j] = src_widen(X[j]);
}

// CSR source -> dense staging rows (already zeroed) of the caller's element type: one wave per row, the lanes stride over
// the row's entries (index and value loads are coalesced), every lane stores one element.  V types the values by size
// only (the bits are copied: -0.0 stays -0.0), I = int / long long.  Entry positions are indptr[r] - base, clamped to
// [0, cnt) in 64 bits before anything is indexed with them; a column index is compared in 64 bits with [0, ds) and with
// the entry before it (canonical CSR: strictly increasing) BEFORE it reaches an address.  An entry that fails is not
// written: err[0] counts them, err[1] keeps the smallest row (row0 + r) that has one.
template <typename V, typename I>
__global__ __launch_bounds__(256) void k_csr_expand(V* __restrict__ Xc, long long ldc, long long rows, long long ds,
                                                     const I* __restrict__ indptr, const I* __restrict__ indices,
                                                     const V* __restrict__ values, long long base, long long cnt,
                                                     long long row0, u64* err) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    constexpr int WPB = 256 / RBL_WAVE;
    for (long long r = (long long)blockIdx.x * WPB + ((int)threadIdx.x / RBL_WAVE); r < rows; r += (long long)gridDim.x * WPB) {
        long long a = (long long)indptr[r] - base, b = (long long)indptr[r + 1] - base;
        a = a < 0 ? 0 : (a > cnt ? cnt : a);
        b = b < 0 ? 0 : (b > cnt ? cnt : b);
        for (long long k = a + lane; k < b; k += RBL_WAVE) {
            const long long c = (long long)indices[k];
            const long long prev = k > a ? (long long)indices[k - 1] : -1;
            if (c >= 0 && c < ds && c > prev) {
                Xc[r * ldc + c] = values[k];
            } else {
                atomicAdd(&err[0], 1ull);
                atomicMin(&err[1], (u64)(row0 + r));
            }
        }
    }
}

template <typename V>
int csr_expand_V(int index_type, void* Xc, long long ldc, long long rows, long long ds, const void* indptr, const void* indices,
                 const void* values, long long base, long long cnt, long long row0, u64* err, int num_cu, hipStream_t s) {
    long long grid = (rows + 3) / 4;
    if (grid > (long long)num_cu * 32) grid = (long long)num_cu * 32;
    if (index_type == RBL_INDEX_I64)
        hipLaunchKernelGGL((k_csr_expand<V, long long>), dim3((unsigned)grid), dim3(256), 0, s, (V*)Xc, ldc, rows, ds,
                           (const long long*)indptr, (const long long*)indices, (const V*)values, base, cnt, row0, err);
    else
        hipLaunchKernelGGL((k_csr_expand<V, int>), dim3((unsigned)grid), dim3(256), 0, s, (V*)Xc, ldc, rows, ds,
                           (const int*)indptr, (const int*)indices, (const V*)values, base, cnt, row0, err);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

template <typename S, typename T>
int form_src_T(void* D, long long ld, long long row0, const void* X, long long ldx, const signed char* ysign, long long rows,
               long long ds, long long d, const double* mean, const double* inv, int num_cu, hipStream_t s, u64* ovf) {
    constexpr int E = StorePkt<T>::E;
    const long long PK = ld / E;
    int tpr_log = 0;
    while ((1LL << tpr_log) < PK && tpr_log < 8) ++tpr_log;
    const long long rpb = 256 >> tpr_log;
    long long grid = (rows + rpb - 1) / rpb;
    if (grid > (long long)num_cu * 32) grid = (long long)num_cu * 32;
    const size_t unit = SrcLoad<S, E>::UNIT;
    const bool vec = ((size_t)(uintptr_t)X % unit == 0) && (((size_t)ldx * sizeof(S)) % unit == 0);
    const bool sc = mean != nullptr;
#define RBL_FORM_SRC(SC_, VEC_)                                                                                          \
    hipLaunchKernelGGL((k_form_src<S, T, SC_, VEC_>), dim3((unsigned)grid), dim3(256), 0, s, (T*)D, ld, row0, (const S*)X, \
                       ldx, ysign, rows, ds, d, mean, inv, tpr_log, ovf)
    if (sc && vec) RBL_FORM_SRC(true, true);
    else if (sc) RBL_FORM_SRC(true, false);
    else if (vec) RBL_FORM_SRC(false, true);
    else RBL_FORM_SRC(false, false);
#undef RBL_FORM_SRC
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}
template <typename S>
int form_src_S(int storage, void* D, long long ld, long long row0, const void* X, long long ldx, const signed char* ysign,
               long long rows, long long ds, long long d, const double* mean, const double* inv, int num_cu, hipStream_t s,
               u64* ovf) {
    if (storage == RBL_STORE_F16)
        return form_src_T<S, rbl_half>(D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
    if (storage == RBL_STORE_F32)
        return form_src_T<S, float>(D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
    return form_src_T<S, double>(D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
}
template <typename S>
int src_colstats_S(const void* X, long long ldx, long long rows, long long ds, const double* shift, double* slab1,
                   double* slab2, long long ld, long long blk0, hipStream_t s) {
    const long long nb = (rows + SRC_STAT_ROWS - 1) / SRC_STAT_ROWS;
    if (nb <= 0 || ds <= 0) return RBL_OK;
    dim3 grid((unsigned)((ds + 255) / 256), (unsigned)(nb < 65535 ? nb : 65535));
    hipLaunchKernelGGL(k_src_colstats<S>, grid, dim3(256), 0, s, (const S*)X, ldx, rows, ds, shift, slab1, slab2, ld, blk0);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

}  // namespace

int64_t src_stat_rows() { return SRC_STAT_ROWS; }

int launch_form_src(int dtype, int storage, void* D, int64_t ld, int64_t row0, const void* X, int64_t ldx,
                    const signed char* ysign, int64_t rows, int64_t ds, int64_t d, const double* mean, const double* inv,
                    int num_cu, hipStream_t s, u64* ovf) {
    if (rows <= 0) return RBL_OK;
    if (dtype == RBL_DTYPE_F16)
        return form_src_S<unsigned short>(storage, D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
    if (dtype == RBL_DTYPE_F32) return form_src_S<float>(storage, D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
    return form_src_S<double>(storage, D, ld, row0, X, ldx, ysign, rows, ds, d, mean, inv, num_cu, s, ovf);
}

int launch_src_colstats(int dtype, const void* X, int64_t ldx, int64_t rows, int64_t ds, const double* shift, double* slab1,
                        double* slab2, int64_t ld, int64_t blk0, hipStream_t s) {
    if (dtype == RBL_DTYPE_F16) return src_colstats_S<unsigned short>(X, ldx, rows, ds, shift, slab1, slab2, ld, blk0, s);
    if (dtype == RBL_DTYPE_F32) return src_colstats_S<float>(X, ldx, rows, ds, shift, slab1, slab2, ld, blk0, s);
    return src_colstats_S<double>(X, ldx, rows, ds, shift, slab1, slab2, ld, blk0, s);
}

int launch_src_colreduce(const double* slab, int64_t nb, int64_t ld, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_colreduce, dim3((unsigned)((ld + 63) / 64)), dim3(1024), 0, s, slab, (int)nb, (long long)ld, out);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_src_row(int dtype, const void* X, int64_t ds, double* out, hipStream_t s) {
    if (ds <= 0) return RBL_OK;
    const unsigned grid = (unsigned)((ds + 255) / 256);
    if (dtype == RBL_DTYPE_F16) hipLaunchKernelGGL(k_src_row<unsigned short>, dim3(grid), dim3(256), 0, s, (const unsigned short*)X, (long long)ds, out);
    else if (dtype == RBL_DTYPE_F32) hipLaunchKernelGGL(k_src_row<float>, dim3(grid), dim3(256), 0, s, (const float*)X, (long long)ds, out);
    else hipLaunchKernelGGL(k_src_row<double>, dim3(grid), dim3(256), 0, s, (const double*)X, (long long)ds, out);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_csr_expand(int dtype, int index_type, void* Xc, int64_t ldc, int64_t rows, int64_t ds, const void* indptr,
                      const void* indices, const void* values, int64_t base, int64_t cnt, int64_t row0, u64* err, int num_cu,
                      hipStream_t s) {
    if (rows <= 0) return RBL_OK;
    const size_t esz = dtype == RBL_DTYPE_F16 ? 2 : dtype == RBL_DTYPE_F32 ? 4 : 8;
    RBL_HIP(hipMemsetAsync(Xc, 0, (size_t)rows * (size_t)ldc * esz, s));   // the implicit entries: +0.0
    if (cnt <= 0) return RBL_OK;
    if (dtype == RBL_DTYPE_F16)
        return csr_expand_V<unsigned short>(index_type, Xc, ldc, rows, ds, indptr, indices, values, base, cnt, row0, err, num_cu, s);
    if (dtype == RBL_DTYPE_F32)
        return csr_expand_V<unsigned int>(index_type, Xc, ldc, rows, ds, indptr, indices, values, base, cnt, row0, err, num_cu, s);
    return csr_expand_V<u64>(index_type, Xc, ldc, rows, ds, indptr, indices, values, base, cnt, row0, err, num_cu, s);
}

int gemvt_slab_rows(int num_cu) { return num_cu * GEMVT_BLOCKS_PER_CU; }

int launch_gemv(int storage, const void* D, int64_t n, int64_t ld, const double* w, double* v, int num_cu,
                hipStream_t s, PassInstance* inst) {
    if (n <= 0) return RBL_OK;
    if (storage == RBL_STORE_CSR) return launch_csr_gemv((const CsrStore*)D, n, w, v, num_cu, s);   // spmv.hip
    if (storage == RBL_STORE_F32) return gemv_T<float>((const float*)D, n, ld, w, v, num_cu, s, inst);
    if (storage == RBL_STORE_F16) return gemv_T<rbl_half>((const rbl_half*)D, n, ld, w, v, num_cu, s, inst);
    return gemv_T<double>((const double*)D, n, ld, w, v, num_cu, s, inst);
}

int launch_gemvt(int storage, const void* D, int64_t n, int64_t ld, const double* c, double* slab, double* q,
                 int num_cu, hipStream_t s, hipEvent_t main_done, size_t slab_doubles, PassInstance* inst) {
    if (n <= 0) {
        RBL_HIP(hipMemsetAsync(q, 0, sizeof(double) * ld, s));
        return RBL_OK;
    }
    // spmv.hip: the slab holds the segments' partial sums
    if (storage == RBL_STORE_CSR) return launch_csr_gemvt((const CsrStore*)D, ld, c, slab, slab_doubles, q, num_cu, s, main_done);
    if (sweep_v_supported(storage, ld)) {
        SweepInstance sq{};
        RBL_TRY(launch_sweep_q(storage, D, n, ld, c, slab, q, num_cu, s, main_done, inst ? &sq : nullptr));
        pass_report(inst, PASS_ROUTE_SWEEP_Q, sq.p, sq.r, sq.s, sq.blocks, 0);
        return RBL_OK;
    }
    int nb = gemvt_blocks(num_cu, n);
    if (storage == RBL_STORE_F32)
        RBL_TRY((gemvt_T<float, false>((const float*)D, n, ld, c, slab, nullptr, nb, s, inst)));
    else if (storage == RBL_STORE_F16)
        RBL_TRY((gemvt_T<rbl_half, false>((const rbl_half*)D, n, ld, c, slab, nullptr, nb, s, inst)));
    else
        RBL_TRY((gemvt_T<double, false>((const double*)D, n, ld, c, slab, nullptr, nb, s, inst)));
    if (main_done) RBL_HIP(hipEventRecord(main_done, s));  // the sweep kernel alone (roofline timing)
    hipLaunchKernelGGL(k_colreduce, dim3((unsigned)((ld + 63) / 64)), dim3(1024), 0, s, slab, nb, (long long)ld, q);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_colstats(int storage, const void* D, int64_t n, int64_t ld, double* slab, double* sum,
                    double* sumsq, int num_cu, hipStream_t s, PassInstance* inst) {
    if (storage == RBL_STORE_F16) {   // the generator takes them from the unrounded draws (synth.hip: launch_synth_stats)
        rbl_set_error("colstats: not available for RBL_STORE_F16");
        return RBL_ERR_INVALID;
    }
    int nb = gemvt_blocks(num_cu, n);
    double* slab2 = slab + (size_t)gemvt_slab_rows(num_cu) * ld;
    if (storage == RBL_STORE_F32)
        RBL_TRY((gemvt_T<float, true>((const float*)D, n, ld, nullptr, slab, slab2, nb, s, inst)));
    else
        RBL_TRY((gemvt_T<double, true>((const double*)D, n, ld, nullptr, slab, slab2, nb, s, inst)));
    hipLaunchKernelGGL(k_colreduce, dim3((unsigned)((ld + 63) / 64)), dim3(1024), 0, s, slab, nb, (long long)ld, sum);
    hipLaunchKernelGGL(k_colreduce, dim3((unsigned)((ld + 63) / 64)), dim3(1024), 0, s, slab2, nb, (long long)ld, sumsq);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_D_to_f64(int storage, const void* D, int64_t ld, int64_t n, int64_t d, double* out, hipStream_t s) {
    long long total = n * d;
    if (total <= 0) return RBL_OK;
    if (storage == RBL_STORE_CSR) {   // D is a descriptor, not rows: rbl_get_D expands chunks with launch_csr_dense
        rbl_set_error("D_to_f64: not available for RBL_STORE_CSR");
        return RBL_ERR_INVALID;
    }
    unsigned grid = (unsigned)((total + 255) / 256);
    if (storage == RBL_STORE_F32)
        hipLaunchKernelGGL(k_D_to_f64<float>, dim3(grid), dim3(256), 0, s, (const float*)D, (long long)ld,
                           (long long)n, (long long)d, out);
    else if (storage == RBL_STORE_F16)
        hipLaunchKernelGGL(k_D_to_f64<rbl_half>, dim3(grid), dim3(256), 0, s, (const rbl_half*)D, (long long)ld,
                           (long long)n, (long long)d, out);
    else
        hipLaunchKernelGGL(k_D_to_f64<double>, dim3(grid), dim3(256), 0, s, (const double*)D, (long long)ld,
                           (long long)n, (long long)d, out);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_standardize_negy(int storage, void* D, int64_t n, int64_t ld, int64_t d, const double* mean,
                            const double* inv_std, const signed char* ysign, hipStream_t s) {
    long long total = n * ld;
    if (total <= 0) return RBL_OK;
    long long nblk = (total + 255) / 256;
    if (nblk > (1 << 20)) nblk = 1 << 20;   // grid-stride kernel: at most 2^28 threads per launch
    if (storage == RBL_STORE_F16) {   // would round twice: the generator writes fp16 matrices in one rounding (synth.hip)
        rbl_set_error("standardize_negy: not available for RBL_STORE_F16");
        return RBL_ERR_INVALID;
    }
    if (storage == RBL_STORE_F32)
        hipLaunchKernelGGL(k_standardize_negy<float>, dim3((unsigned)nblk), dim3(256), 0, s, (float*)D, (long long)n,
                           (long long)ld, (long long)d, mean, inv_std, ysign);
    else
        hipLaunchKernelGGL(k_standardize_negy<double>, dim3((unsigned)nblk), dim3(256), 0, s, (double*)D,
                           (long long)n, (long long)ld, (long long)d, mean, inv_std, ysign);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}
