// synth.hip - synthetic two-class data generated in place on the device, never on the
// host (BASELINE configs C2-C5 do not fit host-side generation + upload).  Reproduces the
// STATISTICS of the reference's synthetic branch, src/util/load_data.py:101-116
// (sklearn make_classification defaults: 2 informative + 2 redundant columns, the other
// d-4 columns N(0,1) noise, 2 clusters per class on hypercube vertices - cluster k belongs to
// class k % 2, its points are standard normal draws times a random matrix A_k with entries
// uniform in (-1, 1), shifted to its vertex at +-class_sep -, redundant = informative @ B,
// flip_y label noise, shuffled columns) followed by preprocessing.scale (done by
// launch_colstats + launch_standardize_negy in sweep.hip).  Counter-based Philox4x32-10,
// keyed by the seed and indexed by (global row, column packet): any sharding of the rows
// over GPUs yields the same matrix.  This kernel writes the RAW matrix (storage type T)
// and the labels; standardisation and the -y scaling follow.
// fp16 storage never holds the raw matrix: the column statistics come from a pass that only regenerates the fp32 draws
// (k_synth_stats), and the matrix is written once as half(-y (x - mean) / std) from draws regenerated again
// (k_synth_f16) - one rounding, so it is the element-wise binary16 rounding of what fp64 storage generates.
#include "rbl_internal.h"

namespace {

struct U4 { unsigned x, y, z, w; };

__device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        unsigned hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        U4 n;
        n.x = hi1 ^ c.y ^ k0;
        n.y = lo1;
        n.z = hi0 ^ c.w ^ k1;
        n.w = lo0;
        c = n;
        k0 += W0;
        k1 += W1;
    }
    return c;
}

__device__ inline float u01(unsigned x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }  // (0,1)

__device__ inline void box_muller(unsigned a, unsigned b, float& n0, float& n1) {
    float r = sqrtf(-2.0f * __logf(u01(a)));
    float s, c;
    __sincosf(6.28318530717958647692f * u01(b), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

struct SynthParams {
    long long n, ld, d, row_offset;
    unsigned k0, k1;
    float class_sep, flip_y;
    int special[4];   // output columns that hold the 2 informative + 2 redundant features
    float mix[4];     // redundant = informative @ mix (2 x 2)
    float A[4][4];    // cluster k: informative = (g0, g1) @ A_k (2 x 2, row-major) + centroid_k
    float cen[4][2];  // centroid of cluster k: its hypercube vertex at +-class_sep
};

// the four raw values of column packet pk of local row r and the row's label (0 / 1)
__device__ inline void synth_packet(const SynthParams& P, long long r, long long pk, float (&x)[4], int& ylab_out) {
    {
        const unsigned long long gr = (unsigned long long)(r + P.row_offset);
        U4 ctr = {(unsigned)gr, (unsigned)(gr >> 32), (unsigned)pk, 1u};
        U4 rnd = philox4x32_10(ctr, P.k0, P.k1);
        box_muller(rnd.x, rnd.y, x[0], x[1]);
        box_muller(rnd.z, rnd.w, x[2], x[3]);
        // per-row draw: label, cluster, flip, informative noise
        U4 rc = {(unsigned)gr, (unsigned)(gr >> 32), 0xFFFFFFFFu, 0u};
        U4 rr = philox4x32_10(rc, P.k0, P.k1);
        const int y01 = rr.x & 1u, cl = (rr.x >> 1) & 1u;
        int ylab = y01;
        if (u01(rr.y) < P.flip_y) ylab = (rr.x >> 2) & 1u;  // sklearn: flipped rows get a random class
        bool touches = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) touches |= (P.special[k] >> 2) == pk;
        if (touches) {
            float g0, g1;
            box_muller(rr.z, rr.w, g0, g1);
            const int c = (cl << 1) | y01;                             // cluster: class = c % 2 as in make_classification
            const float f0 = g0 * P.A[c][0] + g1 * P.A[c][2] + P.cen[c][0];
            const float f1 = g0 * P.A[c][1] + g1 * P.A[c][3] + P.cen[c][1];
            const float feat[4] = {f0, f1, f0 * P.mix[0] + f1 * P.mix[2], f0 * P.mix[1] + f1 * P.mix[3]};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((P.special[k] >> 2) == pk) x[P.special[k] & 3] = feat[k];
        }
        ylab_out = ylab;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_synth(T* __restrict__ D, SynthParams P, signed char* __restrict__ ysign) {
    const long long packets = P.ld / 4;
    const long long total = P.n * packets;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / packets, pk = i - r * packets;
        float x[4];
        int ylab;
        synth_packet(P, r, pk, x, ylab);
        T* dst = D + r * P.ld + pk * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = (pk * 4 + k < P.d) ? (T)x[k] : (T)0;
        if (pk == 0) ysign[r] = ylab ? 1 : -1;
    }
}

// fp16 storage, pass 1: labels and the column sums / sums of squares of the raw draws (fp64 sums of the fp32 values, as
// the column statistics of a stored fp32 / fp64 raw matrix are).  Thread `tid` of column tile blockIdx.y owns one
// 4-column packet over the block's contiguous row range; one slab row per block, summed in a fixed order.
__global__ __launch_bounds__(256) void k_synth_stats(SynthParams P, signed char* __restrict__ ysign, double* __restrict__ slab,
                                                       double* __restrict__ slab2) {
    const long long packets = P.ld / 4;
    const long long pk = (long long)blockIdx.y * 256 + threadIdx.x;
    if (pk >= packets) return;
    const long long rows_per_block = (P.n + gridDim.x - 1) / gridDim.x;
    const long long r_begin = (long long)blockIdx.x * rows_per_block;
    long long r_end = r_begin + rows_per_block;
    if (r_end > P.n) r_end = P.n;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r_begin; r < r_end; ++r) {
        float x[4];
        int ylab;
        synth_packet(P, r, pk, x, ylab);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = (pk * 4 + k < P.d) ? (double)x[k] : 0.0;
            sum[k] += a;
            sq[k] += a * a;
        }
        if (pk == 0) ysign[r] = ylab ? 1 : -1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        slab[(long long)blockIdx.x * P.ld + pk * 4 + k] = sum[k];
        slab2[(long long)blockIdx.x * P.ld + pk * 4 + k] = sq[k];
    }
}
__global__ __launch_bounds__(256) void k_synth_colreduce(const double* __restrict__ slab, int nb, long long ld, double* __restrict__ out) {
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    if (col >= ld) return;
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += slab[(long long)b * ld + col];
    out[col] = acc;
}

// fp16 storage, pass 2: one thread per 16-byte packet of D (two generator packets); the standardised, -y scaled value
// is formed in fp64 exactly as k_standardize_negy forms it and rounded to binary16 once
__global__ __launch_bounds__(256) void k_synth_f16(uint4* __restrict__ D, SynthParams P, const double* __restrict__ mean,
                                                     const double* __restrict__ inv_std) {
    const long long packets = P.ld / 8;
    const long long total = P.n * packets;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / packets, pk8 = i - r * packets;
        unsigned short h[8];
#pragma unroll
        for (int half_pk = 0; half_pk < 2; ++half_pk) {
            float x[4];
            int ylab;
            synth_packet(P, r, pk8 * 2 + half_pk, x, ylab);
            const double ys = ylab ? 1.0 : -1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long j = pk8 * 8 + half_pk * 4 + k;
                double val = 0.0;
                if (j < P.d) {
                    const double xs = ((double)x[k] - mean[j]) * inv_std[j];
                    val = -ys * xs;
                }
                h[half_pk * 4 + k] = f64_to_f16_bits(val);
            }
        }
        D[i] = make_uint4((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16),
                          (unsigned)h[4] | ((unsigned)h[5] << 16), (unsigned)h[6] | ((unsigned)h[7] << 16));
    }
}

SynthParams synth_params(int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed, double class_sep, double flip_y,
                         const int* special, const double* mix, const double* A16, const int* vertex) {
    SynthParams P;
    P.n = n;
    P.ld = ld;
    P.d = d;
    P.row_offset = row_offset;
    P.k0 = (unsigned)seed;
    P.k1 = (unsigned)(seed >> 32);
    P.class_sep = (float)class_sep;
    P.flip_y = (float)flip_y;
    for (int k = 0; k < 4; ++k) {
        P.special[k] = special[k];
        P.mix[k] = (float)mix[k];
        for (int j = 0; j < 4; ++j) P.A[k][j] = (float)A16[4 * k + j];
        P.cen[k][0] = (float)class_sep * ((vertex[k] & 1) ? 1.0f : -1.0f);
        P.cen[k][1] = (float)class_sep * ((vertex[k] & 2) ? 1.0f : -1.0f);
    }
    return P;
}

}  // namespace

int synth_stats_rows(int num_cu) { return gemvt_slab_rows(num_cu); }   // the handle's slab holds two such blocks of ld doubles

int launch_synth_stats(int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed, double class_sep, double flip_y,
                       const int* special, const double* mix, const double* A16, const int* vertex, signed char* ysign,
                       double* slab, double* sum, double* sumsq, int num_cu, hipStream_t s) {
    const SynthParams P = synth_params(n, ld, d, row_offset, seed, class_sep, flip_y, special, mix, A16, vertex);
    if (n <= 0) {
        RBL_HIP(hipMemsetAsync(sum, 0, sizeof(double) * ld, s));
        RBL_HIP(hipMemsetAsync(sumsq, 0, sizeof(double) * ld, s));
        return RBL_OK;
    }
    long long nb = synth_stats_rows(num_cu);
    const long long cap = (n + 63) / 64;   // at least 64 rows per block
    if (nb > cap) nb = cap;
    double* slab2 = slab + (size_t)synth_stats_rows(num_cu) * ld;
    const unsigned ytiles = (unsigned)((ld / 4 + 255) / 256);
    hipLaunchKernelGGL(k_synth_stats, dim3((unsigned)nb, ytiles), dim3(256), 0, s, P, ysign, slab, slab2);
    const unsigned cg = (unsigned)((ld + 255) / 256);
    hipLaunchKernelGGL(k_synth_colreduce, dim3(cg), dim3(256), 0, s, (const double*)slab, (int)nb, (long long)ld, sum);
    hipLaunchKernelGGL(k_synth_colreduce, dim3(cg), dim3(256), 0, s, (const double*)slab2, (int)nb, (long long)ld, sumsq);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_synth_f16(void* D, int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed, double class_sep, double flip_y,
                     const int* special, const double* mix, const double* A16, const int* vertex, const double* mean,
                     const double* inv_std, hipStream_t s) {
    const SynthParams P = synth_params(n, ld, d, row_offset, seed, class_sep, flip_y, special, mix, A16, vertex);
    const long long total = n * (ld / 8);
    if (total <= 0) return RBL_OK;
    long long g = (total + 255) / 256;
    if (g > (1 << 22)) g = 1 << 22;
    hipLaunchKernelGGL(k_synth_f16, dim3((unsigned)g), dim3(256), 0, s, (uint4*)D, P, mean, inv_std);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_synth(int storage, void* D, int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed,
                 double class_sep, double flip_y, const int* special, const double* mix, const double* A16,
                 const int* vertex, signed char* ysign, hipStream_t s) {
    if (storage == RBL_STORE_F16) {
        rbl_set_error("launch_synth: RBL_STORE_F16 is generated by launch_synth_stats + launch_synth_f16");
        return RBL_ERR_INVALID;
    }
    const SynthParams P = synth_params(n, ld, d, row_offset, seed, class_sep, flip_y, special, mix, A16, vertex);
    long long total = n * (ld / 4);
    if (total <= 0) return RBL_OK;
    long long g = (total + 255) / 256;
    if (g > (1 << 22)) g = 1 << 22;
    if (storage == RBL_STORE_F32)
        hipLaunchKernelGGL(k_synth<float>, dim3((unsigned)g), dim3(256), 0, s, (float*)D, P, ysign);
    else
        hipLaunchKernelGGL(k_synth<double>, dim3((unsigned)g), dim3(256), 0, s, (double*)D, P, ysign);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}
