// spmv.hip - RBL_STORE_CSR: D = -y X kept as its non-zero entries.  The forming kernel of rbl_set_data_csr (checks and
// stores the entries of a chunk), the column-form build, v = D w on the row form, q = D^T c on the column form without
// float atomics, both for up to four problems per read of the entries (groups), the dense expansion of row chunks (rbl_get_D, the Gram matrix) and G = D^T D - through the fp64 MFMA
// kernel of gram.hip, or from the entries (spgram.hip) where the rule of csr_gram_plan.h says so.  Every sum has a fixed order that depends on the data and on (n, ld) alone ("Sparse
// storage").
#include "rbl_internal.h"
#include "csr_gram_plan.h"
#include <cstdlib>
#include <vector>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WPB = SP_THREADS / RBL_WAVE;

__device__ inline double sp_widen(double x) { return x; }
__device__ inline double sp_widen(float x) { return (double)x; }
__device__ inline double sp_widen(unsigned short bits) { return (double)(float)__builtin_bit_cast(_Float16, bits); }

// The entries of source rows [row0, row0 + rows) -> the handle's row form.  optr is the handle's own indptr (all n + 1
// entries, built on the host from the checked copy of the source's): row R owns the slots [optr[R], optr[R + 1]), the last
// of them the column of ones' when `ones` is set, and its source entries sit at optr[R] - (ones ? R : 0) - base of the
// chunk's slices of indices / values (clamped to [0, cnt) before anything is indexed).  One wave per row, the lanes
// stride over the entries.  The rules of k_csr_expand, tested before anything is stored: 0 <= column < ds in 64 bits, and
// above the entry before it.  An entry that fails is not written: err[0] counts them, err[1] keeps the smallest row.
template <typename V, typename I>
__global__ __launch_bounds__(SP_THREADS) void k_csr_store(const int64_t* __restrict__ optr, int* __restrict__ col,
                                                          double* __restrict__ val, long long rows, long long row0, long long ds,
                                                          int ones, const I* __restrict__ indices, const V* __restrict__ values,
                                                          long long base, long long cnt, const signed char* __restrict__ ysign,
                                                          u64* err) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long r = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); r < rows; r += (long long)gridDim.x * SP_WPB) {
        const long long R = row0 + r;
        const long long o0 = optr[R], o1 = optr[R + 1];
        long long len = o1 - o0 - (ones ? 1 : 0);
        long long a = o0 - (ones ? R : 0) - base;
        a = a < 0 ? 0 : (a > cnt ? cnt : a);
        if (len > cnt - a) len = cnt - a;
        const bool pos = ysign[R] > 0;
        for (long long k = lane; k < len; k += RBL_WAVE) {
            const long long c = (long long)indices[a + k];
            const long long prev = k > 0 ? (long long)indices[a + k - 1] : -1;
            if (c >= 0 && c < ds && c > prev) {
                const double x = sp_widen(values[a + k]);
                col[o0 + k] = (int)c;
                val[o0 + k] = pos ? -x : x;   // -y_r x, exact
            } else {
                atomicAdd(&err[0], 1ull);
                atomicMin(&err[1], (u64)R);
            }
        }
        if (ones && lane == 0 && o1 > o0) {
            col[o1 - 1] = (int)ds;   // column d - 1
            val[o1 - 1] = pos ? -1.0 : 1.0;
        }
    }
}

// v = D w: a group of L lanes owns a row.  Every lane runs an fp64 FMA chain over its entries k = a + l, a + l + L, ... in
// entry order (col / val loads are coalesced, w is gathered), then a fixed butterfly over the L lanes; lane 0 stores.
// An empty row gives +0.0.  done (optional): a device flag of the caller's - set, the launch is a no-op (the passes an
// operator w-step has enqueued behind its convergence, wstep_op.hip).
template <int L>
__global__ __launch_bounds__(SP_THREADS) void k_csr_gemv(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                         const double* __restrict__ val, const double* __restrict__ w,
                                                         double* __restrict__ v, long long n, const int* __restrict__ done) {
    if (done && *done) return;
    const int l = (int)threadIdx.x & (L - 1);
    constexpr int GPB = SP_THREADS / L;
    for (long long r = (long long)blockIdx.x * GPB + ((int)threadIdx.x / L); r < n; r += (long long)gridDim.x * GPB) {
        const long long a = indptr[r], b = indptr[r + 1];
        double acc = 0.0;
        for (long long k = a + l; k < b; k += L) acc = fma(val[k], w[col[k]], acc);
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, L);
        if (l == 0) v[r] = acc;
    }
}

// q = D^T c, first kernel: one wave sums one segment of a column's entry list (csc_plan.h: every lane looks the segment
// up in the ld + 1 numbers of segptr) - per lane one FMA chain over the entries begin + lane, begin + lane + 64, ... in
// entry order, c gathered by row, then the butterfly over the wave.
__global__ __launch_bounds__(SP_THREADS) void k_csc_segments(const int64_t* __restrict__ colptr, const int64_t* __restrict__ segptr,
                                                             const int* __restrict__ row, const double* __restrict__ cval,
                                                             const double* __restrict__ c, double* __restrict__ part,
                                                             long long ld, long long nseg, int T, const int* __restrict__ done) {
    if (done && *done) return;   // (as in k_csr_gemv)
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long s = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); s < nseg; s += (long long)gridDim.x * SP_WPB) {
        const CscSegment g = csc_segment(colptr, segptr, ld, s, T);
        double acc = 0.0;
        for (long long k = g.begin + lane; k < g.end; k += RBL_WAVE) acc = fma(cval[k], c[row[k]], acc);
#pragma unroll
        for (int off = RBL_WAVE / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, RBL_WAVE);
        if (lane == 0) part[s] = acc;
    }
}

// second kernel: 16 lanes per column add its segments' partial sums - lane l takes the segments first + l, first + l + 16,
// ... in segment order, then the butterfly.  Columns without entries and the padding [d, ld) give +0.0.
constexpr int SP_QL = 16;
__global__ __launch_bounds__(SP_THREADS) void k_csc_columns(const int64_t* __restrict__ segptr, const double* __restrict__ part,
                                                            double* __restrict__ q, long long ld, const int* __restrict__ done) {
    if (done && *done) return;   // (as in k_csr_gemv)
    const int l = (int)threadIdx.x & (SP_QL - 1);
    const long long j = ((long long)blockIdx.x * SP_THREADS + (int)threadIdx.x) / SP_QL;
    if (j >= ld) return;   // (whole groups leave together)
    double acc = 0.0;
    for (long long s = segptr[j] + l; s < segptr[j + 1]; s += SP_QL) acc += part[s];
#pragma unroll
    for (int off = SP_QL / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, SP_QL);
    if (l == 0) q[j] = acc;
}

// ---- the two passes for up to RBL_MULTI_KMAX problems per read of the entries (groups, rbl_decide_multi).  Column k of
// a launch runs the chain of the single-column kernel above on its own accumulator - the same entries in the same order,
// the same butterfly - so it has that kernel's bits; only the loads of (col, val) / (row, cval) are shared.
template <int KC>
struct SpIn {
    const double* p[KC];
};
template <int KC>
struct SpOut {
    double* p[KC];
};

// v_k = D w_k, k < KC: the w_k are gathered through their own pointers (ld doubles each: they stay in L2)
template <int L, int KC>
__global__ __launch_bounds__(SP_THREADS) void k_csr_gemv_multi(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                               const double* __restrict__ val, SpIn<KC> w, SpOut<KC> v, long long n) {
    const int l = (int)threadIdx.x & (L - 1);
    constexpr int GPB = SP_THREADS / L;
    for (long long r = (long long)blockIdx.x * GPB + ((int)threadIdx.x / L); r < n; r += (long long)gridDim.x * GPB) {
        const long long a = indptr[r], b = indptr[r + 1];
        double acc[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k] = 0.0;
        for (long long e = a + l; e < b; e += L) {
            const double x = val[e];
            const int j = col[e];
#pragma unroll
            for (int k = 0; k < KC; ++k) acc[k] = fma(x, w.p[k][j], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
#pragma unroll
            for (int off = L / 2; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, L);
        }
        if (l == 0) {
#pragma unroll
            for (int k = 0; k < KC; ++k) v.p[k][r] = acc[k];
        }
    }
}

// Cp[i * KS + k] = c_k[i], k < KC: the members' c interleaved row by row with stride KS (2 or 4), so that the line the
// q pass gathers for an entry carries every column.  KC = 3 runs at KS = 4: the fourth slot is written +0.0 (whole
// 32-byte rows) and never enters a sum.
template <int KS, int KC>
__global__ void k_pack_cols(SpIn<KC> c, double* __restrict__ Cp, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double x[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) x[k] = k < KC ? c.p[k < KC ? k : 0][i] : 0.0;
        double2* out = reinterpret_cast<double2*>(Cp + i * KS);
#pragma unroll
        for (int k = 0; k < KS; k += 2) out[k / 2] = make_double2(x[k], x[k + 1]);
    }
}

// q_k = D^T c_k, first kernel: k_csc_segments with KC chains per lane; the KC values of a row come from one (KS = 2) or
// two (KS = 4) aligned 16-byte loads of the packed c.  part[s * KS + k]: segment s of member k.
template <int KS, int KC>
__global__ __launch_bounds__(SP_THREADS) void k_csc_segments_multi(const int64_t* __restrict__ colptr, const int64_t* __restrict__ segptr,
                                                                   const int* __restrict__ row, const double* __restrict__ cval,
                                                                   const double* __restrict__ Cp, double* __restrict__ part,
                                                                   long long ld, long long nseg, int T) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long s = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); s < nseg; s += (long long)gridDim.x * SP_WPB) {
        const CscSegment g = csc_segment(colptr, segptr, ld, s, T);
        double acc[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k] = 0.0;
        for (long long e = g.begin + lane; e < g.end; e += RBL_WAVE) {
            const double x = cval[e];
            const double2* cr = reinterpret_cast<const double2*>(Cp + (long long)row[e] * KS);
            double c[KS];
#pragma unroll
            for (int k = 0; k < KS; k += 2) {
                const double2 t = cr[k / 2];
                c[k] = t.x;
                c[k + 1] = t.y;
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) acc[k] = fma(x, c[k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
#pragma unroll
            for (int off = RBL_WAVE / 2; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, RBL_WAVE);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < KC; ++k) part[s * KS + k] = acc[k];
        }
    }
}

// second kernel: k_csc_columns per member - q_k[j] for every j < ld, the padding included
template <int KS, int KC>
__global__ __launch_bounds__(SP_THREADS) void k_csc_columns_multi(const int64_t* __restrict__ segptr, const double* __restrict__ part,
                                                                  SpOut<KC> q, long long ld) {
    const int l = (int)threadIdx.x & (SP_QL - 1);
    const long long j = ((long long)blockIdx.x * SP_THREADS + (int)threadIdx.x) / SP_QL;
    if (j >= ld) return;   // (whole groups leave together)
    double acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = 0.0;
    for (long long s = segptr[j] + l; s < segptr[j + 1]; s += SP_QL) {
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k] += part[s * KS + k];
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
#pragma unroll
        for (int off = SP_QL / 2; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, SP_QL);
    }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) q.p[k][j] = acc[k];
    }
}

// ---- column form: a stable sort of (column, entry id) puts every column's entries in ascending row order
__global__ void k_csc_keys(const int* __restrict__ col, long long nnz, u32* __restrict__ keys, u32* __restrict__ ids) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x) {
        keys[k] = (u32)col[k];
        ids[k] = (u32)k;
    }
}
// colptr[j] = number of entries in columns below j: the first position of the sorted columns that is >= j
__global__ void k_csc_colptr(const u32* __restrict__ sorted_col, long long nnz, int64_t* __restrict__ colptr, long long ld) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > ld) return;
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)sorted_col[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    colptr[j] = lo;
}
// entry ids[p] of the row form -> slot p of the column form; its row: the last r with indptr[r] <= id
__global__ void k_csc_gather(const u32* __restrict__ ids, long long nnz, const int64_t* __restrict__ indptr, long long n,
                             const double* __restrict__ val, int* __restrict__ row, double* __restrict__ cval) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (long long)gridDim.x * blockDim.x) {
        const long long e = (long long)ids[p];
        long long lo = 0, hi = n;   // indptr[lo] <= e < indptr[hi]
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if (indptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        row[p] = (int)lo;
        cval[p] = val[e];
    }
}

// rows [row0, row0 + rows) -> dense fp64 rows of stride ldo (zeroed by the launcher): one wave per row
__global__ __launch_bounds__(SP_THREADS) void k_csr_dense(const int64_t* __restrict__ indptr, const int* __restrict__ col,
                                                          const double* __restrict__ val, long long row0, long long rows,
                                                          long long ldo, double* __restrict__ out) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long r = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); r < rows; r += (long long)gridDim.x * SP_WPB) {
        const long long a = indptr[row0 + r], b = indptr[row0 + r + 1];
        for (long long k = a + lane; k < b; k += RBL_WAVE) out[r * ldo + col[k]] = val[k];
    }
}

__global__ void k_add_into(double* __restrict__ G, const double* __restrict__ Gc, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) G[i] += Gc[i];
}

// ---- scale-only standardisation (rbl_set_centering(h, 0)): the column statistics from the entries, then the scaling
// the source's x of slot p of the column form: the stored value is -y_r x, and -y_r (-y_r x) = x exactly
__device__ inline double sp_source_x(const int* __restrict__ row, const double* __restrict__ cval,
                                     const signed char* __restrict__ ysign, long long p) {
    const double v = cval[p];
    return ysign[row[p]] > 0 ? -v : v;
}
__device__ inline double sp_stat_term(double v, int r, const signed char* __restrict__ ysign, double sh, double mu, bool squares) {
    double t = (ysign[r] > 0 ? -v : v) - sh;
    if (!squares) return t;
    t -= mu;
    return t * t;
}
// One wave per segment of a column's entry list (csc_plan.h), as in k_csc_segments.  PASS 1: part[s] = sum (x - sh);
// PASS 2: part[s] = sum ((x - sh) - mu[col])^2.  sh is the column's first stored x where the column is full (n entries:
// the shift of the dense statistics, a constant column sums exact zeros) and 0 elsewhere.  Lane l runs one chain of plain
// adds over the entries begin + 2l, begin + 2l + 1, begin + 2l + 128, ... in that order, then the butterfly over the wave:
// the order is a function of the column's entries and T alone.  Where the segment begins on an even slot the pair comes
// from one 16-byte load of cval and one 8-byte load of row; an odd beginning reads the same pair element by element.
template <int PASS>
__global__ __launch_bounds__(SP_THREADS) void k_csc_stat_segments(const int64_t* __restrict__ colptr, const int64_t* __restrict__ segptr,
                                                                  const int* __restrict__ row, const double* __restrict__ cval,
                                                                  const signed char* __restrict__ ysign, const double* __restrict__ mu,
                                                                  double* __restrict__ part, long long ld, long long nseg, int T,
                                                                  long long n) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long s = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); s < nseg; s += (long long)gridDim.x * SP_WPB) {
        const CscSegment g = csc_segment(colptr, segptr, ld, s, T);
        const long long c0 = colptr[g.col];
        const double sh = colptr[g.col + 1] - c0 == n ? sp_source_x(row, cval, ysign, c0) : 0.0;
        const double m = PASS == 2 ? mu[g.col] : 0.0;
        const bool even = (g.begin & 1) == 0;
        double acc = 0.0;
        for (long long k = g.begin + 2 * lane; k < g.end; k += 2 * RBL_WAVE) {
            const bool two = k + 1 < g.end;
            double v0, v1 = 0.0;
            int r0, r1 = 0;
            if (even && two) {
                const double2 tv = *reinterpret_cast<const double2*>(cval + k);
                const int2 tr = *reinterpret_cast<const int2*>(row + k);
                v0 = tv.x, v1 = tv.y, r0 = tr.x, r1 = tr.y;
            } else {
                v0 = cval[k], r0 = row[k];
                if (two) v1 = cval[k + 1], r1 = row[k + 1];
            }
            acc += sp_stat_term(v0, r0, ysign, sh, m, PASS == 2);
            if (two) acc += sp_stat_term(v1, r1, ysign, sh, m, PASS == 2);
        }
#pragma unroll
        for (int off = RBL_WAVE / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, RBL_WAVE);
        if (lane == 0) part[s] = acc;
    }
}
// val[k] *= inv[col[k]] over the row form (inv: ld doubles, 1.0 for the column of ones and the pad: those keep their bits)
__global__ void k_csr_scale_rows(const int* __restrict__ col, double* __restrict__ val, long long nnz, const double* __restrict__ inv) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x)
        val[k] = val[k] * inv[col[k]];
}
// ... and over the column form: one wave per segment, the column's factor read once
__global__ __launch_bounds__(SP_THREADS) void k_csc_scale_segments(const int64_t* __restrict__ colptr, const int64_t* __restrict__ segptr,
                                                                   double* __restrict__ cval, const double* __restrict__ inv,
                                                                   long long ld, long long nseg, int T) {
    const int lane = (int)threadIdx.x & (RBL_WAVE - 1);
    for (long long s = (long long)blockIdx.x * SP_WPB + ((int)threadIdx.x / RBL_WAVE); s < nseg; s += (long long)gridDim.x * SP_WPB) {
        const CscSegment g = csc_segment(colptr, segptr, ld, s, T);
        const double f = inv[g.col];
        for (long long k = g.begin + lane; k < g.end; k += RBL_WAVE) cval[k] = cval[k] * f;
    }
}

unsigned sp_grid(long long items, long long per_block, int num_cu) {
    long long g = (items + per_block - 1) / per_block;
    const long long cap = (long long)(num_cu > 0 ? num_cu : 256) * 64;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

template <typename V>
int csr_store_V(int index_type, const CsrStore* st, long long rows, long long row0, long long ds, int ones, const void* indices,
                const void* values, long long base, long long cnt, const signed char* ysign, u64* err, int num_cu, hipStream_t s) {
    const unsigned grid = sp_grid(rows, SP_WPB, num_cu);
    if (index_type == RBL_INDEX_I64)
        hipLaunchKernelGGL((k_csr_store<V, long long>), dim3(grid), dim3(SP_THREADS), 0, s, (const int64_t*)st->indptr, st->col, st->val,
                           rows, row0, ds, ones, (const long long*)indices, (const V*)values, base, cnt, ysign, err);
    else
        hipLaunchKernelGGL((k_csr_store<V, int>), dim3(grid), dim3(SP_THREADS), 0, s, (const int64_t*)st->indptr, st->col, st->val,
                           rows, row0, ds, ones, (const int*)indices, (const V*)values, base, cnt, ysign, err);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

}  // namespace

// RBL_CSR_TUNING_HOOKS (a build flag of the measuring tool alone, tools/csr_storage_bench.py --segs / --lanes; never set in
// the library that ships): the lane group and the segment length can then be overridden from the environment at upload.
// Without it L is a function of the data and T the compile-time constant: no environment variable changes the order of
// a sum.
int csr_lanes(int64_t nnz, int64_t n) {
#ifdef RBL_CSR_TUNING_HOOKS
    if (const char* e = getenv("RBL_CSR_LANES")) {
        const int v = atoi(e);
        if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) return v;
    }
#endif
    // the narrowest group whose lanes take at most eight entries of an average row ("Sparse storage": measured)
    const int64_t rows = n > 0 ? n : 1;
    int L = 4;
    while (L < 64 && (int64_t)8 * L * rows < nnz) L *= 2;
    return L;
}

int csr_store_reserve(DevArena& mem, CsrStore* st, int64_t n, int64_t ld, int64_t nnz, bool columns) {
    if (!st->indptr) RBL_TRY(mem.alloc(&st->indptr, (size_t)n + 1));   // (each on its own: a failed call is made up for by the next)
    if (columns && !st->colptr) RBL_TRY(mem.alloc(&st->colptr, (size_t)ld + 1));
    if (columns && !st->segptr) RBL_TRY(mem.alloc(&st->segptr, (size_t)ld + 1));
    if (!st->col || !st->val || (columns && (!st->row || !st->cval)) || st->cap != nnz) {   // a second upload regrows the entry buffers
        for (void* p : {(void*)st->col, (void*)st->val, (void*)st->row, (void*)st->cval})
            if (p) mem.release(p);
        st->col = st->row = nullptr;
        st->val = st->cval = nullptr;
        st->cap = 0;
        RBL_TRY(mem.alloc(&st->col, (size_t)nnz));
        RBL_TRY(mem.alloc(&st->val, (size_t)nnz));
        if (columns) {
            RBL_TRY(mem.alloc(&st->row, (size_t)nnz));
            RBL_TRY(mem.alloc(&st->cval, (size_t)nnz));
        }
        st->cap = nnz;
    }
    st->n = n;
    st->nnz = nnz;
    st->nseg = 0;
    return RBL_OK;
}

int launch_csr_store(int dtype, int index_type, const CsrStore* st, int64_t rows, int64_t row0, int64_t ds, int ones,
                     const void* indices, const void* values, int64_t base, int64_t cnt, const signed char* ysign, u64* err,
                     int num_cu, hipStream_t s) {
    if (rows <= 0) return RBL_OK;
    if (dtype == RBL_DTYPE_F16)
        return csr_store_V<unsigned short>(index_type, st, rows, row0, ds, ones, indices, values, base, cnt, ysign, err, num_cu, s);
    if (dtype == RBL_DTYPE_F32)
        return csr_store_V<float>(index_type, st, rows, row0, ds, ones, indices, values, base, cnt, ysign, err, num_cu, s);
    return csr_store_V<double>(index_type, st, rows, row0, ds, ones, indices, values, base, cnt, ysign, err, num_cu, s);
}

int csr_store_finish(CsrStore* st, int64_t ld, bool columns, int num_cu, hipStream_t s) {
    // st->lanes (cleared when the upload began) says "complete" to every pass, a borrower's included: it is set as the
    // last step, once the column form and its segment table stand
    const int64_t n = st->n, nnz = st->nnz;
    const int lanes = csr_lanes(nnz, n);
    st->lanes = 0;
    st->seg = CSC_SEG;
#ifdef RBL_CSR_TUNING_HOOKS
    if (const char* e = getenv("RBL_CSC_SEG")) {
        const int v = atoi(e);
        if (v >= 64 && v <= 2048 && (v & (v - 1)) == 0) st->seg = v;
    }
#endif
    st->nseg = 0;
    if (!columns) {
        st->lanes = lanes;
        return RBL_OK;
    }
    std::vector<int64_t> cp((size_t)ld + 1, 0), sp((size_t)ld + 1, 0);
    if (nnz > 0) {
        DevArena tmp;   // the sort's workspace: freed before the call returns (after the stream wait)
        SortWorkspace ws{};
        u64 *k0 = nullptr, *k1 = nullptr;
        RBL_TRY(tmp.alloc(&k0, (size_t)(nnz + 1) / 2));   // nnz 32-bit keys each
        RBL_TRY(tmp.alloc(&k1, (size_t)(nnz + 1) / 2));
        ws.keys[0] = k0, ws.keys[1] = k1;
        RBL_TRY(tmp.alloc(&ws.vals[0], (size_t)nnz));
        RBL_TRY(tmp.alloc(&ws.vals[1], (size_t)nnz));
        RBL_TRY(tmp.alloc((unsigned char**)&ws.spine, sort_spine_bytes()));
        RBL_TRY(tmp.alloc(&ws.bin_total, 256));
        RBL_TRY(tmp.alloc(&ws.bin_base, 256));
        RBL_TRY(tmp.alloc((unsigned char**)&ws.ghist, sort_ghist_bytes()));
        RBL_HIP(hipMemsetAsync(ws.ghist, 0, sort_ghist_bytes(), s));
        u32* keys = reinterpret_cast<u32*>(k0);
        hipLaunchKernelGGL(k_csc_keys, dim3(sp_grid(nnz, 256, num_cu)), dim3(256), 0, s, (const int*)st->col, (long long)nnz, keys,
                           ws.vals[0]);
        int rc = launch_radix_sort32(ws, nnz, s);
        if (rc == RBL_OK) {
            hipLaunchKernelGGL(k_csc_colptr, dim3((unsigned)((ld + 1 + 255) / 256)), dim3(256), 0, s, (const u32*)keys, (long long)nnz,
                               st->colptr, (long long)ld);
            hipLaunchKernelGGL(k_csc_gather, dim3(sp_grid(nnz, 256, num_cu)), dim3(256), 0, s, (const u32*)ws.vals[0], (long long)nnz,
                               (const int64_t*)st->indptr, (long long)n, (const double*)st->val, st->row, st->cval);
            if (hipGetLastError() != hipSuccess) rc = RBL_ERR_HIP;
        }
        if (rc == RBL_OK && hipMemcpyAsync(cp.data(), st->colptr, sizeof(int64_t) * (size_t)(ld + 1), hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = RBL_ERR_HIP;
        if (hipStreamSynchronize(s) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
        if (rc == RBL_ERR_HIP) rbl_set_error("set_data_csr: building the column form failed: %s", hipGetErrorString(hipGetLastError()));
        RBL_TRY(rc);
    } else {
        RBL_HIP(hipMemsetAsync(st->colptr, 0, sizeof(int64_t) * (size_t)(ld + 1), s));
    }
    const int64_t nseg = csc_plan_segptr(cp.data(), ld, st->seg, sp.data());
    RBL_HIP(hipMemcpyAsync(st->segptr, sp.data(), sizeof(int64_t) * (size_t)(ld + 1), hipMemcpyHostToDevice, s));
    RBL_HIP(hipStreamSynchronize(s));
    st->nseg = nseg;
    st->lanes = lanes;
    return RBL_OK;
}

int launch_csr_gemv(const CsrStore* st, int64_t n, const double* w, double* v, int num_cu, hipStream_t s, const int* done) {
    if (n <= 0) return RBL_OK;
#define RBL_CSR_GEMV(L_)                                                                                                      \
    hipLaunchKernelGGL(k_csr_gemv<L_>, dim3(sp_grid(n, SP_THREADS / L_, num_cu)), dim3(SP_THREADS), 0, s, (const int64_t*)st->indptr, \
                       (const int*)st->col, (const double*)st->val, w, v, (long long)n, done)
    switch (st->lanes) {
        case 4: RBL_CSR_GEMV(4); break;
        case 8: RBL_CSR_GEMV(8); break;
        case 16: RBL_CSR_GEMV(16); break;
        case 32: RBL_CSR_GEMV(32); break;
        case 64: RBL_CSR_GEMV(64); break;
        default: rbl_set_error("csr gemv: the data are not complete (no upload, or the last one failed)"); return RBL_ERR_STATE;
    }
#undef RBL_CSR_GEMV
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_csr_gemvt(const CsrStore* st, int64_t ld, const double* c, double* part, size_t part_doubles, double* q, int num_cu,
                     hipStream_t s, hipEvent_t main_done, const int* done) {
    if (!st->colptr || !st->segptr) {
        rbl_set_error("csr gemvt: the handle holds the row form only (objective-only)");
        return RBL_ERR_STATE;
    }
    if (!st->lanes) {   // (an upload that failed half way: the entry buffers hold nothing to be read)
        rbl_set_error("csr gemvt: the data are not complete (the last upload failed)");
        return RBL_ERR_STATE;
    }
    if ((size_t)st->nseg > part_doubles) {
        rbl_set_error("csr gemvt: the slab holds %zu partial sums, the data have %lld segments", part_doubles, (long long)st->nseg);
        return RBL_ERR_STATE;
    }
    if (st->nseg > 0)
        hipLaunchKernelGGL(k_csc_segments, dim3(sp_grid(st->nseg, SP_WPB, num_cu)), dim3(SP_THREADS), 0, s, (const int64_t*)st->colptr,
                           (const int64_t*)st->segptr, (const int*)st->row, (const double*)st->cval, c, part, (long long)ld,
                           (long long)st->nseg, st->seg, done);
    if (main_done) RBL_HIP(hipEventRecord(main_done, s));   // the pass over the entries alone (roofline timing)
    hipLaunchKernelGGL(k_csc_columns, dim3((unsigned)((ld * SP_QL + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, s,
                       (const int64_t*)st->segptr, (const double*)part, q, (long long)ld, done);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

namespace {

template <int KC>
int csr_gemv_multi_K(const CsrStore* st, int64_t n, const double* const* w, double* const* v, int num_cu, hipStream_t s) {
    SpIn<KC> wi;
    SpOut<KC> vo;
    for (int k = 0; k < KC; ++k) {
        wi.p[k] = w[k];
        vo.p[k] = v[k];
    }
#define RBL_CSR_GEMV_MULTI(L_)                                                                                           \
    hipLaunchKernelGGL((k_csr_gemv_multi<L_, KC>), dim3(sp_grid(n, SP_THREADS / L_, num_cu)), dim3(SP_THREADS), 0, s,        \
                       (const int64_t*)st->indptr, (const int*)st->col, (const double*)st->val, wi, vo, (long long)n)
    switch (st->lanes) {
        case 4: RBL_CSR_GEMV_MULTI(4); break;
        case 8: RBL_CSR_GEMV_MULTI(8); break;
        case 16: RBL_CSR_GEMV_MULTI(16); break;
        case 32: RBL_CSR_GEMV_MULTI(32); break;
        case 64: RBL_CSR_GEMV_MULTI(64); break;
        default: rbl_set_error("csr gemv multi: the data are not complete (no upload, or the last one failed)"); return RBL_ERR_STATE;
    }
#undef RBL_CSR_GEMV_MULTI
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

template <int KS, int KC>
int csr_gemvt_multi_K(const CsrStore* st, int64_t n, int64_t ld, const double* const* c, double* Cp, double* part, double* const* q,
                      int num_cu, hipStream_t s, hipEvent_t pack_done) {
    SpIn<KC> ci;
    SpOut<KC> qo;
    for (int k = 0; k < KC; ++k) {
        ci.p[k] = c[k];
        qo.p[k] = q[k];
    }
    hipLaunchKernelGGL((k_pack_cols<KS, KC>), dim3(sp_grid(n, 256, num_cu)), dim3(256), 0, s, ci, Cp, (long long)n);
    if (pack_done) RBL_HIP(hipEventRecord(pack_done, s));   // the interleaving alone (tools/csr_group_bench.py)
    if (st->nseg > 0)
        hipLaunchKernelGGL((k_csc_segments_multi<KS, KC>), dim3(sp_grid(st->nseg, SP_WPB, num_cu)), dim3(SP_THREADS), 0, s,
                           (const int64_t*)st->colptr, (const int64_t*)st->segptr, (const int*)st->row, (const double*)st->cval,
                           (const double*)Cp, part, (long long)ld, (long long)st->nseg, st->seg);
    hipLaunchKernelGGL((k_csc_columns_multi<KS, KC>), dim3((unsigned)((ld * SP_QL + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, s,
                       (const int64_t*)st->segptr, (const double*)part, qo, (long long)ld);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

}  // namespace

int csr_multi_stride(int k) { return k <= 2 ? 2 : 4; }

int launch_csr_gemv_multi(const CsrStore* st, int64_t n, int k, const double* const* w, double* const* v, int num_cu, hipStream_t s) {
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("csr gemv multi: 1..%d columns per launch (got %d)", RBL_MULTI_KMAX, k);
        return RBL_ERR_INVALID;
    }
    if (n <= 0) return RBL_OK;
    if (!st->lanes) {
        rbl_set_error("csr gemv multi: the data are not complete (no upload, or the last one failed)");
        return RBL_ERR_STATE;
    }
    switch (k) {
        case 1: return launch_csr_gemv(st, n, w[0], v[0], num_cu, s);
        case 2: return csr_gemv_multi_K<2>(st, n, w, v, num_cu, s);
        case 3: return csr_gemv_multi_K<3>(st, n, w, v, num_cu, s);
        default: return csr_gemv_multi_K<4>(st, n, w, v, num_cu, s);
    }
}

int launch_csr_gemvt_multi(const CsrStore* st, int64_t n, int64_t ld, int k, const double* const* c, double* Cp, size_t cp_doubles,
                           double* part, size_t part_doubles, double* const* q, int num_cu, hipStream_t s, hipEvent_t pack_done) {
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("csr gemvt multi: 1..%d columns per launch (got %d)", RBL_MULTI_KMAX, k);
        return RBL_ERR_INVALID;
    }
    if (!st->colptr || !st->segptr) {
        rbl_set_error("csr gemvt multi: the handle holds the row form only (objective-only)");
        return RBL_ERR_STATE;
    }
    if (!st->lanes) {
        rbl_set_error("csr gemvt multi: the data are not complete (the last upload failed)");
        return RBL_ERR_STATE;
    }
    if (k == 1) {
        if (n <= 0) return RBL_OK;
        return launch_csr_gemvt(st, ld, c[0], part, part_doubles, q[0], num_cu, s, nullptr);
    }
    const size_t ks = (size_t)csr_multi_stride(k);
    if ((size_t)st->nseg * ks > part_doubles) {
        rbl_set_error("csr gemvt multi: the slab holds %zu partial sums, the data have %lld segments of %zu columns", part_doubles,
                      (long long)st->nseg, ks);
        return RBL_ERR_STATE;
    }
    if (n > 0 && (size_t)(n > st->n ? n : st->n) * ks > cp_doubles) {   // (the entries' row ids index it)
        rbl_set_error("csr gemvt multi: the packed c holds %zu doubles, %lld rows of %zu columns are needed", cp_doubles, (long long)n, ks);
        return RBL_ERR_STATE;
    }
    if (n <= 0) return RBL_OK;
    switch (k) {
        case 2: return csr_gemvt_multi_K<2, 2>(st, n, ld, c, Cp, part, q, num_cu, s, pack_done);
        case 3: return csr_gemvt_multi_K<4, 3>(st, n, ld, c, Cp, part, q, num_cu, s, pack_done);
        default: return csr_gemvt_multi_K<4, 4>(st, n, ld, c, Cp, part, q, num_cu, s, pack_done);
    }
}

int launch_csr_dense(const CsrStore* st, int64_t row0, int64_t rows, int64_t ldo, double* out, int num_cu, hipStream_t s) {
    if (rows <= 0 || ldo <= 0) return RBL_OK;
    if (!st->lanes) {   // (no upload yet, or one that failed half way: col may hold anything - nothing is indexed with it)
        rbl_set_error("csr dense: the data are not complete (no upload, or the last one failed)");
        return RBL_ERR_STATE;
    }
    RBL_HIP(hipMemsetAsync(out, 0, sizeof(double) * (size_t)rows * (size_t)ldo, s));   // the implicit entries: +0.0
    if (st->nnz <= 0) return RBL_OK;
    hipLaunchKernelGGL(k_csr_dense, dim3(sp_grid(rows, SP_WPB, num_cu)), dim3(SP_THREADS), 0, s, (const int64_t*)st->indptr,
                       (const int*)st->col, (const double*)st->val, (long long)row0, (long long)rows, (long long)ldo, out);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_csr_colstats(const CsrStore* st, int64_t n, int64_t ld, const signed char* ysign, int pass, const double* mu,
                        double* part, double* sums, int num_cu, hipStream_t s) {
    if (!st->colptr || !st->segptr || !st->lanes) {
        rbl_set_error("csr column statistics: the handle holds no complete column form");
        return RBL_ERR_STATE;
    }
    if (pass != 1 && pass != 2) {
        rbl_set_error("csr column statistics: pass must be 1 or 2 (got %d)", pass);
        return RBL_ERR_INVALID;
    }
    if (st->nseg > 0) {
        const dim3 grid(sp_grid(st->nseg, SP_WPB, num_cu)), block(SP_THREADS);
        if (pass == 1)
            hipLaunchKernelGGL(k_csc_stat_segments<1>, grid, block, 0, s, (const int64_t*)st->colptr, (const int64_t*)st->segptr,
                               (const int*)st->row, (const double*)st->cval, ysign, mu, part, (long long)ld, (long long)st->nseg,
                               st->seg, (long long)n);
        else
            hipLaunchKernelGGL(k_csc_stat_segments<2>, grid, block, 0, s, (const int64_t*)st->colptr, (const int64_t*)st->segptr,
                               (const int*)st->row, (const double*)st->cval, ysign, mu, part, (long long)ld, (long long)st->nseg,
                               st->seg, (long long)n);
    }
    // the segments' sums of a column, folded as q = D^T c folds them (16 lanes per column, then the butterfly)
    hipLaunchKernelGGL(k_csc_columns, dim3((unsigned)((ld * SP_QL + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, s,
                       (const int64_t*)st->segptr, (const double*)part, sums, (long long)ld, (const int*)nullptr);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int launch_csr_scale(const CsrStore* st, int64_t ld, const double* inv, int num_cu, hipStream_t s) {
    if (!st->lanes) {
        rbl_set_error("csr scale: the data are not complete (no upload, or the last one failed)");
        return RBL_ERR_STATE;
    }
    if (st->nnz <= 0) return RBL_OK;
    hipLaunchKernelGGL(k_csr_scale_rows, dim3(sp_grid(st->nnz, 256, num_cu)), dim3(256), 0, s, (const int*)st->col, st->val,
                       (long long)st->nnz, inv);
    if (st->colptr && st->segptr && st->cval && st->nseg > 0)
        hipLaunchKernelGGL(k_csc_scale_segments, dim3(sp_grid(st->nseg, SP_WPB, num_cu)), dim3(SP_THREADS), 0, s,
                           (const int64_t*)st->colptr, (const int64_t*)st->segptr, st->cval, inv, (long long)ld, (long long)st->nseg,
                           st->seg);
    RBL_HIP(hipGetLastError());
    return RBL_OK;
}

int64_t csr_gram_chunk_rows(int64_t n, int64_t ld) {
    int64_t rows = (256LL << 20) / (8 * (ld > 0 ? ld : 1));
    rows = rows / 8 * 8;
    if (rows < 8) rows = 8;
    return rows < n ? rows : n;
}

int launch_csr_gram(const CsrStore* st, int64_t n, int64_t ld, int64_t d, double* slab, double* G, int num_cu, hipStream_t s,
                    int route, int tile_cols, rbl_gram_report* rep) {
    if (route != 0 && route != CSR_GRAM_ROUTE_DENSE && route != CSR_GRAM_ROUTE_SPARSE) {
        rbl_set_error("csr gram: route must be 0 (the rule's), 2 (dense expansion) or 3 (from the entries), got %d", route);
        return RBL_ERR_INVALID;
    }
    if (rep) {
        *rep = rbl_gram_report{};
        rep->pair_products = st->pair_products;
        rep->dense_products = csr_gram_dense_products(n, ld);
    }
    if (n <= 0) {
        if (rep) rep->route = CSR_GRAM_ROUTE_DENSE;
        return launch_gram(RBL_STORE_F64, nullptr, 0, ld, d, slab, G, num_cu, s);
    }
    if (route == 0) route = csr_gram_route(n, ld, st->pair_products);
    if (route == CSR_GRAM_ROUTE_SPARSE) return launch_csr_spgram(st, n, ld, G, num_cu, tile_cols, s, rep);
    const int64_t chunk = csr_gram_chunk_rows(n, ld);
    DevArena tmp;   // the staging rows and the chunk's G: freed on return, after the stream wait
    double *stage = nullptr, *Gc = nullptr;
    RBL_TRY(tmp.alloc(&stage, (size_t)chunk * (size_t)ld));
    if (chunk < n) RBL_TRY(tmp.alloc(&Gc, (size_t)ld * (size_t)ld));
    int rc = RBL_OK;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (rep) {
        RBL_HIP(hipEventCreate(&ev[0]));
        if (hipEventCreate(&ev[1]) != hipSuccess || hipEventRecord(ev[0], s) != hipSuccess) rc = RBL_ERR_HIP;
    }
    for (int64_t r0 = 0; r0 < n && rc == RBL_OK; r0 += chunk) {
        const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
        rc = launch_csr_dense(st, r0, rows, ld, stage, num_cu, s);
        if (rc == RBL_OK) rc = launch_gram(RBL_STORE_F64, stage, rows, ld, d, slab, r0 == 0 ? G : Gc, num_cu, s);
        if (rc == RBL_OK && r0 > 0) {   // G += the chunk's, in chunk order
            const long long cnt = (long long)ld * ld;
            hipLaunchKernelGGL(k_add_into, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, G, (const double*)Gc, cnt);
            if (hipGetLastError() != hipSuccess) rc = RBL_ERR_HIP;
        }
    }
    if (rep && rc == RBL_OK && hipEventRecord(ev[1], s) != hipSuccess) rc = RBL_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
    if (rep && rc == RBL_OK) {
        rep->route = CSR_GRAM_ROUTE_DENSE;
        rep->transient_bytes = (int64_t)sizeof(double) * (chunk * ld + (chunk < n ? ld * ld : 0));
        if (hipEventElapsedTime(&rep->ms, ev[0], ev[1]) != hipSuccess) rc = RBL_ERR_HIP;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc == RBL_ERR_HIP) rbl_set_error("csr gram: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}
