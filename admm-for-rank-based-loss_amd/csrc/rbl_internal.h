// rbl_internal.h - shared declarations of librbl.so (gfx950 only, no portability layer).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "../../include/rbl.h"
#include "wset_plan.h"

void rbl_set_error(const char* fmt, ...);

// Host wait for a word in pinned memory that a kernel writes last (after __threadfence_system):
// spins on the word; after 2 s without a change the stream is waited for instead, so that a
// failed launch cannot hang the host.
void rbl_spin_wait(const volatile int* word, int sentinel, hipStream_t stream);
// every host wait for the device inside an iteration is counted (rbl_stats.host_syncs); rbl_spin_wait counts itself
void rbl_note_host_sync();

#define RBL_HIP(x)                                                                         \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            rbl_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            return RBL_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define RBL_TRY(x)                 \
    do {                           \
        int r_ = (x);              \
        if (r_ != RBL_OK) return r_; \
    } while (0)

// Launchers that pick a kernel instance by the loss id: STMT is compiled once per loss with the constant L_ = the id;
// any other id is an error of the caller (rbl_create checks the configuration, the rbl_k_* entry points their argument).
#define RBL_LOSS_SWITCH(loss, L_, ...)                                \
    do {                                                              \
        switch (loss) {                                               \
            case RBL_LOSS_BCE: {                                      \
                constexpr int L_ = RBL_LOSS_BCE;                      \
                __VA_ARGS__;                                          \
            } break;                                                  \
            case RBL_LOSS_HINGE: {                                    \
                constexpr int L_ = RBL_LOSS_HINGE;                    \
                __VA_ARGS__;                                          \
            } break;                                                  \
            case RBL_LOSS_SQHINGE: {                                  \
                constexpr int L_ = RBL_LOSS_SQHINGE;                  \
                __VA_ARGS__;                                          \
            } break;                                                  \
            default:                                                  \
                rbl_set_error("unknown loss id %d", (int)(loss));     \
                return RBL_ERR_INVALID;                               \
        }                                                             \
    } while (0)

// RBL_OK for an id RBL_LOSS_SWITCH dispatches on, else RBL_ERR_INVALID with the message set: the one list of losses that
// rbl_create's check of the configuration and the rbl_k_* entry points share with the launchers
inline int rbl_check_loss(int loss) {
    RBL_LOSS_SWITCH(loss, L_, return (void)L_, RBL_OK);
    return RBL_OK;
}

// Owner of device (hipMalloc) and pinned host (hipHostMalloc) buffers: its destructor frees every buffer
// allocated through it.  One per solver / baseline handle, or a local one for scoped temporaries.
class DevArena {
  public:
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() {
        for (const Buf& b : bufs_) (void)(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    }
    // count == 0 allocates one element; on failure *p = NULL, the error text is set and RBL_ERR_NOMEM returned
    template <typename T>
    int alloc(T** p, size_t count) {
        *p = nullptr;
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)p, count * sizeof(T));
        if (e != hipSuccess) {
            rbl_set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
            return RBL_ERR_NOMEM;
        }
        bufs_.push_back({*p, false});
        return RBL_OK;
    }
    // pinned host memory the device accesses directly (flags as hipHostMalloc takes them)
    template <typename T>
    int pinned(T** p, size_t count, unsigned flags) {
        *p = nullptr;
        RBL_HIP(hipHostMalloc((void**)p, count * sizeof(T), flags));
        bufs_.push_back({*p, true});
        return RBL_OK;
    }
    // frees one buffer ahead of the others (a buffer that is regrown)
    void release(void* p) {
        for (size_t i = 0; i < bufs_.size(); ++i)
            if (bufs_[i].p == p) {
                (void)(bufs_[i].pinned ? hipHostFree(p) : hipFree(p));
                bufs_.erase(bufs_.begin() + (long)i);
                return;
            }
    }

  private:
    struct Buf {
        void* p;
        bool pinned;
    };
    std::vector<Buf> bufs_;
};

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int RBL_WAVE = 64;

// ---- RBL_STORE_F16: IEEE binary16 elements ----------------------------------------------------------------------
// The kernels read halves as bit patterns out of 16-byte packets and widen them half -> float -> double (both exact);
// rbl_half only types the pointers.  Every write of a half goes through f64_to_f16_bits: ONE round-to-nearest-even from
// the fp64 value (integer arithmetic, the same on host and device - NumPy's float64 -> float16 conversion bit for bit),
// subnormals kept, overflow to +-inf (the callers count those: rbl_set_data_from rejects them).
typedef _Float16 rbl_half;
__host__ __device__ inline unsigned short f64_to_f16_bits(double x) {
    const u64 b = __builtin_bit_cast(u64, x);
    const unsigned sign = (unsigned)(b >> 48) & 0x8000u;
    const int e = (int)((b >> 52) & 0x7ff);
    const u64 m = b & ((1ull << 52) - 1);
    if (e == 0x7ff) return (unsigned short)(sign | 0x7c00u | (m ? 0x200u : 0u));   // inf / nan
    const int he = e - 1023 + 15;                                                 // biased binary16 exponent
    if (he >= 31) return (unsigned short)(sign | 0x7c00u);
    if (e == 0 || he < -11) return (unsigned short)sign;                          // below half the smallest subnormal
    const int shift = he > 0 ? 42 : 43 - he;                                      // bits dropped (subnormals: more)
    const u64 mant = m | (1ull << 52);
    u64 r = mant >> shift;
    const u64 rem = mant & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    // normal: r carries the implicit bit (1024 .. 2048), a carry moves into the exponent (and to inf from he = 30)
    return (unsigned short)(sign | (unsigned)(he > 0 ? ((u64)(he - 1) << 10) + r : r));
}
__host__ __device__ inline bool f16_bits_inf(unsigned short h) { return (h & 0x7fffu) == 0x7c00u; }
// the row stride: whole 16-byte packets, zero padded
inline int64_t rbl_storage_ld(int storage, int64_t d) {
    const int64_t e = storage == RBL_STORE_F16 ? 8 : 4;
    return (d + e - 1) / e * e;
}
inline size_t rbl_storage_esz(int storage) { return storage == RBL_STORE_F16 ? 2 : storage == RBL_STORE_F32 ? 4 : 8; }
inline int rbl_storage_packet(int storage) { return storage == RBL_STORE_F16 ? 8 : storage == RBL_STORE_F32 ? 4 : 2; }   // elements per 16 bytes
constexpr int PAV_CHUNK_LOG = 10;              // prefix-sum chunk = 1024 sorted positions
constexpr int PAV_CHUNK = 1 << PAV_CHUNK_LOG;

// ---- two-level prefix sums over sorted positions (pav.hip) -------------------------
// P(i) = sum_{j<i} x_j = (cph[i>>10] + cpl[i>>10]) + locx[i]; locx restarts at every
// 1024-chunk so that small-block sums do not cancel against n-sized prefixes.
struct Prefix {
    const double* locx;  // n+1 entries, exclusive prefix inside the chunk
    const double* cph;   // chunk-level exclusive prefix, double-double high part
    const double* cpl;   //                               double-double low part
};
// the buffers behind one Prefix (api.hip: alloc_prefix)
struct PrefixBufs {
    double* locx = nullptr;    // n+1
    double* chunk = nullptr;   // nchunks: chunk totals
    double* cph = nullptr;     // nchunks
    double* cpl = nullptr;     // nchunks
    Prefix view() const { return Prefix{locx, cph, cpl}; }
};

struct SeamRec {
    long long s;  // first pooled position, -1: no merge
    long long e;  // last pooled position
    double x;     // pooled value
};

// ---- sweep.hip ------------------------------------------------------------------------
// which kernel instance launch_gemv / launch_gemvt / launch_colstats ran (optional trailing out-parameter: the
// rbl_k_pass_* entry points report it, the solver leaves it NULL; RBL_STORE_CSR does not fill it).
//   route PASS_ROUTE_PLAIN, k_gemv:   a = LPR lanes per row, p = P passes (0: w staged in LDS), u = U row groups in flight,
//                                     blocks launched, tiles = 1
//   route PASS_ROUTE_PLAIN, k_gemvt:  a = TPR threads per row, p = PJ packets per thread, u = U steps in flight, blocks =
//                                     row blocks nb (slab rows), tiles = column tiles (gridDim.y)
//   route PASS_ROUTE_SWEEP_Q:         launch_gemvt handed the pass to launch_sweep_q: a, p, u, blocks = the SweepInstance's
//                                     p, r, s, blocks; tiles = 0
enum { PASS_ROUTE_PLAIN = 0, PASS_ROUTE_SWEEP_Q = 1 };
struct PassInstance {
    int route, a, p, u, blocks, tiles;
};
inline void pass_report(PassInstance* inst, int route, int a, int p, int u, int blocks, int tiles) {
    if (inst) *inst = PassInstance{route, a, p, u, blocks, tiles};
}
// v = D w : D is n x ld row-major (ld % 4 == 0, fp16 storage: ld % 8 == 0; columns >= d are zero)
int launch_gemv(int storage, const void* D, int64_t n, int64_t ld, const double* w, double* v,
                int num_cu, hipStream_t s, PassInstance* inst = nullptr);
// q = D^T c : partial column sums go to slab (gemvt_slab_rows() x ld doubles), then q
int gemvt_slab_rows(int num_cu);
// RBL_STORE_CSR: the slab holds one partial sum per segment; slab_doubles is what it has room for (a slab too small is
// RBL_ERR_STATE, never a write past its end)
int launch_gemvt(int storage, const void* D, int64_t n, int64_t ld, const double* c, double* slab,
                 double* q, int num_cu, hipStream_t s, hipEvent_t main_done = nullptr, size_t slab_doubles = 0,
                 PassInstance* inst = nullptr);
int launch_D_to_f64(int storage, const void* D, int64_t ld, int64_t n, int64_t d, double* out,
                    hipStream_t s);
// column sums / sums of squares (slab-reduced, deterministic) and in-place standardisation
int launch_colstats(int storage, const void* D, int64_t n, int64_t ld, double* slab, double* sum,
                    double* sumsq, int num_cu, hipStream_t s, PassInstance* inst = nullptr);
int launch_standardize_negy(int storage, void* D, int64_t n, int64_t ld, int64_t d, const double* mean,
                            const double* inv_std, const signed char* ysign, hipStream_t s);
// typed sources (rbl_set_data_from): X of element type dtype (RBL_DTYPE_*) already on the device, ds source columns.
// D[row0 + r][j] = round(-y_r x), x = widen(X[r][j]) or, with mean / inv given (device, ld doubles), (widen - mean[j]) *
// inv[j]; columns ds .. d - 1 are -y_r (the column of ones), the pad zeros.  ysign: the signs of rows row0 .. row0 + rows.
// ovf (RBL_STORE_F16, else NULL): [0] += finite entries that rounded to +-inf, [1] = min of their row * d + column
int launch_form_src(int dtype, int storage, void* D, int64_t ld, int64_t row0, const void* X, int64_t ldx,
                    const signed char* ysign, int64_t rows, int64_t ds, int64_t d, const double* mean, const double* inv,
                    int num_cu, hipStream_t s, u64* ovf);
// shifted column sums sum (x - shift_j), sum (x - shift_j)^2 of row blocks of src_stat_rows() rows -> slab rows blk0 + b
// (ld doubles each); launch_src_colreduce folds nb slab rows in a fixed order; launch_src_row widens one row
int64_t src_stat_rows();
int launch_src_colstats(int dtype, const void* X, int64_t ldx, int64_t rows, int64_t ds, const double* shift, double* slab1,
                        double* slab2, int64_t ld, int64_t blk0, hipStream_t s);
int launch_src_colreduce(const double* slab, int64_t nb, int64_t ld, double* out, hipStream_t s);
int launch_src_row(int dtype, const void* X, int64_t ds, double* out, hipStream_t s);
// CSR source (rbl_set_data_csr) -> `rows` dense rows of stride ldc elements of type dtype in Xc (zeroed here first), which
// the launchers above then read.  indptr: the rows + 1 entries of these rows, of index_type (RBL_INDEX_*); entry positions
// in indices / values are indptr[r] - base, clamped to [0, cnt).  A column index outside [0, ds) or not above the entry
// before it is not written: err[0] += 1, err[1] = min(err[1], row0 + r).
int launch_csr_expand(int dtype, int index_type, void* Xc, int64_t ldc, int64_t rows, int64_t ds, const void* indptr,
                      const void* indices, const void* values, int64_t base, int64_t cnt, int64_t row0, u64* err, int num_cu,
                      hipStream_t s);

// ---- elementwise.hip --------------------------------------------------------------------
// rs (optional, in the launchers below): the sign vector of a handle with labels of its own on a borrowed D
// (rbl_set_labels): r_i = y_i * y_owner_i.  v, z, lambda, c are then in the owner's sign convention, m is the true m.
// sigma_rows != NULL (row weights): the prox of row i runs with sigma_rows[i] in the place of sigma0
int launch_erm_zc(int loss, int64_t n, double sigma0, double rho, const double* v, const double* lam,
                  double* m, double* z, double* c, hipStream_t s, const signed char* rs = nullptr,
                  const double* sigma_rows = nullptr);
// m = v - lambda/rho together with the sort's input: keys[i] = order-preserving transform of m[i], idx[i] = i + idx_off
int launch_make_m_keys(int64_t n, double rho, const double* v, const double* lam, double* m, u64* keys, u32* idx,
                       u32 idx_off, hipStream_t s, const signed char* rs = nullptr);
int launch_keys_from_m(int64_t n, const double* m, u64* keys, u32* idx, hipStream_t s);
// z-step with 32-bit sort keys (round 3): m and its range; the fixed-point keys; after the sort, sorted m / row ids with
// the runs of equal keys put in (m, row) order (*flag = 1: a run too long - sort 64-bit keys instead)
int s32_range_words();   // u64 words of the range buffer mm
int launch_make_m_range(int64_t n, double rho, const double* v, const double* lam, double* m, u64* mm, hipStream_t s,
                        const signed char* rs = nullptr);
int launch_keys32(int64_t n, const double* m, const u64* mm, u32* keys, u32* idx, u32 idx_off, hipStream_t s);
int launch_sort32_fix(int64_t n, const u32* keys, const u32* ids, const double* m, u32 off, double* ms, u32* ids_out, int* flag,
                      hipStream_t s);
int launch_prox(int loss, int64_t n, const double* sigma, double rho, const double* m, double* out,
                hipStream_t s);
// lambda += rho (z - v); partial sums {sum (z-v)^2, sum loss(v)} -> red[0..1]
int launch_dual(int loss, int64_t n, double rho, const double* z, const double* v, double* lam,
                double* partials, double* red, hipStream_t s);
int launch_accuracy(int loss, int64_t n, const double* v, const signed char* ysign, double tau, double* partials,
                    double* out, hipStream_t s, const signed char* rs = nullptr);
int launch_fair_counts(int64_t n, const double* v, const signed char* ysign, const double* group, double threshold,
                       double* partials, double* out14, hipStream_t s, const signed char* rs = nullptr);
// row-wise arg-max of the scores -ysign_i * V[j][i] over columns j0 .. j0 + kk - 1 (V: kk x n) against best / cls so far
int launch_decide_rows(int64_t n, int kk, int j0, const double* V, const signed char* ysign, double* best, int* cls,
                       hipStream_t s);
int launch_weights(int wf, int64_t n, const double* args, double* alphas, double* betas, hipStream_t s);
// generic deterministic two-stage reduction helpers
int reduce_blocks();
int launch_sum_partials(const double* partials, int nblocks, int K, double* out, hipStream_t s);
// losses of v (for the objective), optionally as sortable keys
int launch_loss_keys(int64_t n, const double* v, u64* keys, hipStream_t s, const signed char* rs = nullptr);
int launch_sorted_loss_dot(int loss, int64_t n, const u64* sorted_keys, const double* sigma,
                           double* partials, double* out, hipStream_t s);
// cw != NULL (row weights): scale * sum_i cw[i] * loss_i, the same two stages in the same order
int launch_loss_sum(int loss, int64_t n, const double* v, double scale, double* partials, double* out,
                    hipStream_t s, const signed char* rs = nullptr, const double* cw = nullptr);

// ---- sort.hip -------------------------------------------------------------------------
struct SortWorkspace {
    u64* keys[2];
    u32* vals[2];
    u32* spine;      // 256 * RS_MAX_BLOCKS
    u32* bin_total;  // 256
    u32* bin_base;   // 256
    u32* ghist;      // the spine scan's done-counter (zero between launches)
};
size_t sort_spine_bytes();
size_t sort_ghist_bytes();
// sorts keys[0]/vals[0] ascending (stable); result ends in keys[0]/vals[0]
// key_bits: number of low key bits that can differ (digits above are skipped)
int launch_radix_sort(SortWorkspace& ws, int64_t n, bool with_vals, hipStream_t s, int key_bits = 64);
int launch_radix_sort32(SortWorkspace& ws, int64_t n, hipStream_t s);
// api.hip: the workspace for n keys (and values) in mem; the done-counter is zeroed on s
int alloc_sort(DevArena& mem, SortWorkspace& sw, int64_t n, bool with_vals, hipStream_t s);

// ---- pav.hip ----------------------------------------------------------------------------
// ex (round 3, optional): the upper levels in one persistent launch (bar / big / num_cu) and, for a single-handle EHRM
// z-step, the branch speculated from the previous iteration with the singleton-stage sums formed inside the bottom
// kernel (fpart / spec / B; `branch` is then WRITTEN by the exact test before the upper levels read it).
enum { PAV_UPPER_DEFAULT = 0, PAV_UPPER_PERSIST = 1, PAV_UPPER_TWO_LAUNCH = 2 };
struct PavExtras {
    unsigned* bar;      // pav_bar_uints() counters, zeroed at allocation
    int bar_parity;     // flips per launch
    SeamRec* big;       // pav_big_recs(n) entries: long pooled ranges all blocks fill together
    int num_cu;
    double* fpart;      // pav_fpart_doubles(n): per-tile shares of the two sums (NULL: no speculation)
    int spec;           // speculated branch (0 = a, 1 = b)
    double B;
    int upper;          // upper levels: PAV_UPPER_DEFAULT (RBL_PAV_UPPER_PERSIST decides, persistent unless it is 0),
                        // PAV_UPPER_PERSIST (k_pav_upper) or PAV_UPPER_TWO_LAUNCH (k_pav_seam_wave + k_pav_fill per level)
};
size_t pav_bar_uints();
int rbl_live_handles(int device);   // api.hip: solver handles of this process alive on a device
int64_t pav_big_recs(int64_t n);   // n: the most positions the workspace's PAV sees
int64_t pav_fpart_doubles(int64_t n);
constexpr int PAV_LEVEL_FILLS = 4;
constexpr int PAV_COUNTERS = PAV_LEVEL_FILLS + 64;
struct PavWorkspace {
    double* ms;        // n   sorted m
    double* u;         // n   current block values by sorted position
    PrefixBufs pm;     // prefix sums of ms
    SeamRec* recs;     // seams of the upper levels
    u32* counters;     // PAV_COUNTERS: [0] merges, [1] dirty upper levels, [2] long fills, [3] status of the persistent
                       // upper-level kernel, [PAV_LEVEL_FILLS + l] long fills of upper level l
    double* partials;  // reduce scratch
    int* branch;       // EHRM branch flag on the device (0 = a, 1 = b)
    PavExtras ex;      // round-3 paths of launch_pav_tree (buffers owned by this workspace)
};
int64_t pav_num_chunks(int64_t n);
int64_t pav_num_recs(int64_t n);
int launch_prefix(const double* x, int64_t n, const PrefixBufs& p, hipStream_t s);
int launch_unflip_keys(int64_t n, const u64* keys, double* ms, hipStream_t s);
int launch_unflip_prefix(const u64* keys, int64_t n, double* ms, const PrefixBufs& p, hipStream_t s);
// EHRM: scalar branch test (PAV_cpt.py:205-226) -> *branch
// u0a / u0b (optional): the element prox of both branches is kept for launch_pav_tree
int launch_ehrm_branch(int64_t n, const double* sa, const double* sb, double B, double rho, const double* ms,
                       double* partials, int* branch, int forced, hipStream_t s, double* u0a = nullptr,
                       double* u0b = nullptr);
// element prox (level 0) + merge tree -> u.  sigma = sa, or sb when *branch != 0 (EHRM); the
// matching prefix sums are pa / pb.
// u0a / u0b != NULL: level 0 (element prox of branch a / b) was computed already; u0a may alias u
int launch_pav_tree(int loss, int64_t n, double rho, const double* ms, const double* sa, const double* sb, double* u,
                    Prefix pa, Prefix pb, Prefix pm, const int* branch, SeamRec* recs, u32* merge_counter,
                    hipStream_t s, const double* u0a = nullptr, const double* u0b = nullptr, PavExtras* ex = nullptr);
// z[perm[i]] = clip(u[i]); c[perm[i]] = z + lam[perm[i]]/rho  (local slice [off, off+nloc))
// ---- distributed z-step (merge tree over ranks; pav.hip, CPU restatement oracle/zdist.py)
struct ZdSeam {
    int active, k, side, a0, b1;   // this rank's seam at the current level: id, 0 = left / 1 = right group, rank range
    long long lo, hi, n;           // undecided index range [lo, hi) of the chunk (n positions)
    double x, cnt;                 // pooled block: value and length
};
int launch_ehrm_fvals(int64_t n, const double* sa, const double* sb, double B, double rho, const double* ms,
                      double* partials, double* out2, hipStream_t s, double* u0a = nullptr, double* u0b = nullptr);
int launch_ehrm_pick(const double* fvals_total, int* branch, hipStream_t s);
int launch_add_u32(int64_t n, u32* x, u32 add, hipStream_t s);
int launch_make_c(int64_t n, const double* z, const double* lam, double rho, double* c, hipStream_t s);
int launch_zd_sample(const u64* keys, int64_t n, int ns, double* out, hipStream_t s);
int launch_zd_split_bounds(const u64* keys, int64_t n, const double* split, int nsplit, long long* bounds, hipStream_t s);
int launch_zd_counts_from_bounds(const long long* bounds, int nparts, int64_t n, long long* counts, hipStream_t s);
int launch_zd_bounds(const double* u, int64_t n, double* out3, hipStream_t s);
int launch_zd_seam_setup(int rank, int world, int level, const double* bounds_all, int64_t n, ZdSeam* st, hipStream_t s);
int launch_zd_update_propose(int loss, ZdSeam* st, const double* u, int K, int world, const double* cand_prev,
                             const double* part_prev, double rho, double* cand_out, hipStream_t s);
int launch_zd_eval(const ZdSeam* st, const double* u, Prefix pa, Prefix pb, Prefix pm, const int* branch, int K, int world,
                   const double* cand_all, double* part, hipStream_t s);
int launch_zd_pooled(const ZdSeam* st, Prefix pa, Prefix pb, Prefix pm, const int* branch, int nseams, double* sums, int* err,
                     hipStream_t s);
int launch_zd_fill(int loss, ZdSeam* st, const double* sums_total, double rho, double* u, int64_t n, hipStream_t s);
int launch_zd_ids_to_keys(int64_t n, const u32* ids, u64* keys, u32* pos, hipStream_t s);
int launch_zd_gather_back(int64_t n, const u64* keys_sorted, const u32* pos, const double* u, u32* out_ids, double* out_u,
                          hipStream_t s);
int launch_zd_owner_bounds(const u64* keys_sorted, int64_t n, int64_t nmax, int world, long long* bounds, hipStream_t s);
int launch_zd_scatter(int64_t n, const u32* ids, const double* uu, const int* branch, double B, int has_B, double rho,
                      const double* lam, double* z, double* c, int64_t off, int64_t nloc, hipStream_t s);
int launch_scatter_z(int64_t n, const double* u, const u32* perm, const int* branch, double B, int has_B,
                     double rho, const double* lam, double* z, double* c, int64_t off, int64_t nloc,
                     hipStream_t s, const signed char* rs = nullptr);

// ---- wstep.hip --------------------------------------------------------------------------
constexpr int RBL_GRAM_MAX_LD = 16384;   // the widest ld of the Gram-space w-step (its single-block update kernels)
// which persistent kernel instance a w-step launched (wp_run fills it through WstepWorkspace::inst: the rbl_k_wstep_seq
// entry reports it, the solver leaves the pointer NULL, as with SweepInstance)
struct WstepInstance {
    int glds, per, nblocks, lds_bytes;   // G rows in LDS, vector elements per thread, blocks launched, dynamic LDS
};
struct WstepWorkspace {
    double* yk;     // d
    double* Gy;     // d
    double* wn;     // d
    double* r;      // d (CG)
    double* p;      // d (CG)
    double* scal;   // small device scalars: [0]=t, [1]=rr, ...
    int* flags;     // [0]=done, [1]=iters
    int* pin;       // host-pinned, device-visible: [0..3] = status block of the active-set lasso kernel, [4..5] = CG (done, iterations)
    // l2 w-step: G = V diag(lambda) V^T computed once by rbl_gram_finish (eig.hip); NULL / false: CG
    double *eig_Vt, *eig_V, *eig_lambda;
    bool eig_ok;
    int last_iters; // CG iterations of the previous w-step (sizes the next batch)
    int last_fista; // the same for FISTA; pin[6..7] = its (done, iterations)
    // persistent one-launch w-steps (wstep.hip: k_cg_persist / k_ncg_persist): pin[4..5] / pin[8..9] = their (status,
    // iterations), pin[10] = what became of the nonlinear CG's linear first phase.  The blocks meet through the tagged
    // granules of xch alone (wp_exchange): there are no barrier counters, and nothing is cleared between launches
    unsigned* bar;  // only [0] is used: the abort word of the persistent kernels (a block that gave up waiting)
    double* xch;    // the two exchange buffers of the matrix-vector products: 8-byte granules {tag | 32 bits}, two per double
    int launch_seq; // launches so far (the tags of a launch: launch_seq << 12 | exchange number)
    bool gw_valid;  // ws.Gy holds G w of the w the last run_wstep returned
    int form;       // how the last run_wstep ran (rbl_stats.wstep_form)
    int ncg_skip, ncg_backoff;   // persistent nonlinear CG: w-steps left without / length of the pause of its linear first phase
    // per-coordinate penalties (rbl_set_penalty): device vectors of ld doubles each (padding 0), NULL = the scalar reg;
    // pen_l2max = max_j l2_j (FISTA's step constant)
    const double *pen_l1, *pen_l2;
    double pen_l2max;
    WstepInstance* inst;   // NULL in the solver; the test entry's report of the persistent launch
};
constexpr int WSTEP_BAR_UINTS = 2 * 10 * 32;
constexpr int WSTEP_PERSIST_MAX_LD = 2048;                                  // 8 vector elements per thread of a 256-thread block
constexpr int WSTEP_XCH_GRANULES = 2 * (WSTEP_PERSIST_MAX_LD + 16);        // granules of one exchange buffer
constexpr int WSTEP_XCH_DOUBLES = 2 * WSTEP_XCH_GRANULES;                 // two buffers
int alloc_wstep(DevArena& mem, WstepWorkspace& ww, int64_t ld, hipStream_t s);   // api.hip
int launch_power_iteration(const double* G, int64_t d, double* tmp1, double* tmp2, double* scal, int iters,
                           double* lambda_host, hipStream_t s);
// lasso / smoothed-l1 by FISTA with restart, ridge by CG; w is updated in place.
// If fs_pending != NULL and the w-step is the lasso, only the active-set kernel is enqueued and
// *fs_pending = true is returned: the caller may enqueue work that assumes success, then calls
// finish_wstep_l1(), which waits for the kernel's status and runs FISTA when it did not converge
// (*fell_back = true: w changed again, work enqueued in between must be redone).
int run_wstep(int wstep, const double* G, int64_t d, const double* q, double rho, double reg, double smooth_t,
              double L, double tol, int max_inner, double* w, WstepWorkspace& ws, int* iters_host,
              hipStream_t s, bool* fs_pending = nullptr, const double* rho_dev = nullptr,
              double* w_prev_out = nullptr, bool want_Gw = false);   // want_Gw: the lasso kernel leaves G w in ws.Gy
int finish_wstep_l1(const double* G, int64_t d, const double* q, double rho, double reg, double L, double tol,
                    int max_inner, double* w, WstepWorkspace& ws, int* iters_host, hipStream_t s, bool* fell_back);
// l1 != NULL: pen_out4 = [sum w^2, ||w||_1, sum_j l1_j |w_j|, sum_j l2_j w_j^2] as well
int launch_w_stats(int64_t d, const double* w, const double* w_prev, double* out3, hipStream_t s, const double* l1 = nullptr,
                   const double* l2 = nullptr, double* pen_out4 = nullptr);
// lasso_fs.hip: exact active-set (feature-sign) lasso in one workgroup; out_dev = 4 ints
// rho_dev != NULL: kappa = reg / (2 rho_dev[0]) is formed on the device; w_prev_out != NULL: the warm start is saved there
int launch_lasso_fs(const double* G, int64_t ld, int64_t d, const double* q, double* w, double kappa, int* out_dev,
                    hipStream_t s, const double* rho_dev = nullptr, double reg = 0.0, double* w_prev_out = nullptr,
                    double* Gw_out = nullptr);   // Gw_out: G w of the solution (valid when the status is 0)
int launch_reg_terms(int64_t d, const double* w, double* out2 /* [sum w^2, sum |w|] */, hipStream_t s);
// [sum w^2, sum |w|, sum_j l1_j |w_j|, sum_j l2_j w_j^2]
int launch_pen_terms(int64_t d, const double* w, const double* l1, const double* l2, double* out4, hipStream_t s);
// the active-set kernel's per-coordinate instance: kappa_j = l1[j] / (2 rho), l2[j] / rho on the diagonal; rho from
// rho_dev[0] when given
int launch_lasso_fs_pen(const double* G, int64_t ld, int64_t d, const double* q, double* w, double rho, const double* l1,
                        const double* l2, int* out_dev, hipStream_t s, const double* rho_dev = nullptr,
                        double* w_prev_out = nullptr, double* Gw_out = nullptr);
int launch_soft_threshold(int64_t d, double* w, double t, hipStream_t s);

// which kernel instance a row-streaming launcher ran (optional out-parameter of the launch_sweep_* functions: the
// rbl_k_sweep_* entry points report it, the solver passes NULL).  kind: the wave-per-row kernels (p = P packets per
// lane) or the workgroup-per-row kernel (p = PT packets per thread); r rows per sub-batch, s sub-batches per
// super-batch, blocks launched.
enum { SWEEP_KIND_WAVE = 0, SWEEP_KIND_WIDE = 1 };
struct SweepInstance {
    int kind, p, r, s, blocks;
};
inline void sweep_report(SweepInstance* inst, int kind, int p, int r, int s, int blocks) {
    if (inst) *inst = SweepInstance{kind, p, r, s, blocks};
}

// ---- sweep_erm.hip: one pass over D per iteration for erm (fused dual update + next z-step + D^T c)
bool sweep_erm_supported(int storage, int64_t ld);
int sweep_erm_blocks(int num_cu);
int sweep_erm_slab_rows(int num_cu);
int launch_sweep_erm(int storage, int loss, const void* D, int64_t n, int64_t ld, const double* w, const double* z_old,
                     double* lam, double* v, double* z_new, double sigma0, double rho, const double* pred_dev,
                     double* slab, double* partials, double* q, double* red, double* zz_out, int num_cu, hipStream_t s,
                     hipEvent_t main_done, int want_obj, SweepInstance* inst = nullptr,
                     const double* sigma_rows = nullptr /* n: the row-weighted twins, sigma0 unused */,
                     const double* loss_w = nullptr /* n: row weights of the logged loss sum */);
// the same pass with one sigma per row (sweep_erm_w.hip); called by launch_sweep_erm
int launch_sweep_erm_w(int storage, int loss, const void* D, int64_t n, int64_t ld, const double* w, const double* z_old,
                       double* lam, double* v, double* z_new, const double* sigma_rows, double rho, const double* pred_dev,
                       double* slab, double* partials, double* q, double* red, double* zz_out, int num_cu, hipStream_t s,
                       hipEvent_t main_done, int want_obj, SweepInstance* inst, const double* loss_w);
// rho_{k+1} prediction + the w statistics (||w - w_prev||^2, sum w^2, ||w||_1 -> wstats[0..2]); p_out != p
// rho_dev != NULL: rho is read from rho_dev[0] on the device (may alias pred)
int launch_predict_rho(int64_t ld, const double* q, const double* p, double* p_out, const double* w, const double* w_prev,
                       const double* Gw, const double* zz, double rho, double cap, double* pred, double* wstats,
                       hipStream_t s, const double* rho_dev = nullptr);
int launch_sumsq(int64_t n, const double* x, double* partials, double* out, hipStream_t s);
// v = D w, lambda += rho (z - v), red[0] = sum (z - v)^2 in one pass (rows up to 4 / 8 passes of 64 packets)
bool sweep_v_supported(int storage, int64_t ld);
// q = D^T c with the single-sweep kernel's row-streaming loads (sweep_erm.hip: SE_QONLY) for the widths of
// sweep_v_supported; launch_gemvt routes to it
int launch_sweep_q(int storage, const void* D, int64_t n, int64_t ld, const double* c, double* slab, double* q, int num_cu,
                   hipStream_t s, hipEvent_t main_done, SweepInstance* inst = nullptr);
int launch_sweep_v(int storage, const void* D, int64_t n, int64_t ld, const double* w, const double* z, double* lam,
                   double* v, double rho, double* partials, double* red, int num_cu, hipStream_t s, hipEvent_t main_done,
                   SweepInstance* inst = nullptr);
// ---- sweep_multi.hip: the two passes for up to RBL_MULTI_KMAX problems on one D per launch (widths of sweep_v_supported)
#define RBL_MULTI_KMAX 4
bool sweep_multi_supported(int storage, int64_t ld);
int sweep_multi_k(int storage, int64_t ld);                      // columns one launch carries at this width
size_t sweep_multi_slab_doubles(int64_t ld, int num_cu);         // slab of launch_sweep_q_multi
// v_j = D w_j; z != NULL: also lambda_j += rho_j (z_j - v_j) and red_j[0] = sum (z_j - v_j)^2, red_j[1] = 0
// (partials_j: 3 doubles per CU).  Arrays of k host-side pointers / values, 1 <= k <= RBL_MULTI_KMAX.
int launch_sweep_v_multi(int storage, const void* D, int64_t n, int64_t ld, int k, const double* const* w, const double* const* z,
                         double* const* lam, double* const* v, const double* rho, double* const* partials, double* const* red,
                         int num_cu, hipStream_t s, SweepInstance* inst = nullptr);
// q_j = D^T c_j
int launch_sweep_q_multi(int storage, const void* D, int64_t n, int64_t ld, int k, const double* const* c, double* slab,
                         double* const* q, int num_cu, hipStream_t s, SweepInstance* inst = nullptr);
int launch_symv(const double* G, int64_t ld, const double* x, double* y, hipStream_t s);
int launch_symv_ab(const double* G, int64_t ld, const double* x, double* y, double alpha, double beta, hipStream_t s);   // y = alpha G x + beta x

// ---- eig.hip: one-time eigendecomposition of G for the l2 w-step
int launch_eig_jacobi(const double* G, int64_t ld, int64_t d, double* Bt, double* Vt, double* V, double* lambda,
                      unsigned long long* offmax_dev, hipStream_t s, int* sweeps_out);
int launch_ridge_eig(const double* G, const double* Vt, const double* V, const double* lambda, int64_t ld, const double* q,
                     double rho, double reg, double* w, double* tmp1, double* tmp2, hipStream_t s);

// ---- gram.hip ---------------------------------------------------------------------------
size_t gram_slab_bytes(int64_t d, int num_cu, int64_t n);
// the launch plan of the dense path (optional out-parameter of launch_gram: rbl_k_gram_full reports it): tiles of 128
// columns, tile pairs ti <= tj, row splits (slab tiles per pair) and rows per split
struct GramPlanOut {
    int ntiles, npairs, ksplit;
    long long rows_per_split;
};
int launch_gram(int storage, const void* D, int64_t n, int64_t ld, int64_t d, double* slab, double* G,
                int num_cu, hipStream_t s, GramPlanOut* plan = nullptr);

// ---- spmv.hip: RBL_STORE_CSR - D as its non-zero entries --------------------------------------------------------
// The descriptor a handle's D points at (launch_gemv / launch_gemvt / launch_gram take it as `D` with storage
// RBL_STORE_CSR).  Host memory owned by the arena that owns the buffers (only the host reads it); it never moves:
// borrowers copy the pointer.  Row form: indptr (n + 1), col / val (nnz).  Column form (NULL on an objective-only handle): colptr (ld + 1),
// row / cval (nnz) - every column's entries in ascending row order - and segptr (ld + 1, csc_plan.h).
struct CsrStore {
    int64_t* indptr;
    int* col;
    double* val;
    int64_t* colptr;
    int* row;
    double* cval;
    int64_t* segptr;
    int64_t n, nnz, nseg, cap;   // cap: entries the entry buffers were allocated for
    int lanes;                   // lanes per row of v = D w (csr_lanes), 0 = no data yet
    int seg;                     // entries per segment of q = D^T c
    int64_t pair_products;       // sum_r k_r (k_r + 1) / 2 of the rows as stored (host, from indptr): the Gram route's rule
};
int csr_lanes(int64_t nnz, int64_t n);   // 4 .. 64, from the average row length alone
// (re)allocates the buffers for n rows / nnz entries in mem; the caller then fills indptr and runs launch_csr_store over
// the source's chunks
int csr_store_reserve(DevArena& mem, CsrStore* st, int64_t n, int64_t ld, int64_t nnz, bool columns);
// rows [row0, row0 + rows): the entries at indptr[R] - (ones ? R : 0) - base of indices / values (cnt of them, types as
// launch_csr_expand) are checked (err as there) and stored as (column, -y_R x); ones: the slot (d - 1 = ds, -y_R) as well.
// ysign: the signs of all n rows
int launch_csr_store(int dtype, int index_type, const CsrStore* st, int64_t rows, int64_t row0, int64_t ds, int ones,
                     const void* indices, const void* values, int64_t base, int64_t cnt, const signed char* ysign, u64* err,
                     int num_cu, hipStream_t s);
// after the last chunk: the lane group, and with columns the column form and its segment table; returns with s idle
int csr_store_finish(CsrStore* st, int64_t ld, bool columns, int num_cu, hipStream_t s);
// Scale-only standardisation of a complete store (rbl_set_centering(h, 0)).  Column sums of the source's x = -y_r * value
// from the column form, per column: pass 1 sums[j] = sum (x - sh_j), pass 2 sums[j] = sum ((x - sh_j) - mu[j])^2 over the
// stored entries (sh_j: the first stored x of a full column, else 0).  Two stages - one wave per segment into part
// (st->nseg doubles), then the fold of q = D^T c - in an order that the column's entries and the segment length fix;
// sums: ld doubles (columns without entries and the pad: +0.0); mu (ld doubles) is read by pass 2 alone.
int launch_csr_colstats(const CsrStore* st, int64_t n, int64_t ld, const signed char* ysign, int pass, const double* mu,
                        double* part, double* sums, int num_cu, hipStream_t s);
// every stored value times inv[its column] (ld doubles), row form and - where the handle has one - column form
int launch_csr_scale(const CsrStore* st, int64_t ld, const double* inv, int num_cu, hipStream_t s);
// done (optional, both passes): a device flag - where it is set when a kernel starts, that kernel does nothing (output untouched)
int launch_csr_gemv(const CsrStore* st, int64_t n, const double* w, double* v, int num_cu, hipStream_t s, const int* done = nullptr);
// part: the segments' partial sums, part_doubles >= st->nseg of them (fewer: RBL_ERR_STATE before anything is launched)
int launch_csr_gemvt(const CsrStore* st, int64_t ld, const double* c, double* part, size_t part_doubles, double* q, int num_cu,
                     hipStream_t s, hipEvent_t main_done, const int* done = nullptr);
// The two passes for k problems (1 <= k <= RBL_MULTI_KMAX) per read of the entries; arrays of k host-side pointers.  Column
// j has the bits of the single-column launcher on w[j] / c[j] alone (k = 1 is that launcher); k = 3 runs three chains, on
// the q side over packed rows of four.  v_j = D w_j:
int launch_csr_gemv_multi(const CsrStore* st, int64_t n, int k, const double* const* w, double* const* v, int num_cu, hipStream_t s);
// q_j = D^T c_j (ld entries each).  Cp: the c_j interleaved row by row, written here (k_pack_cols) - csr_multi_stride(k)
// doubles per row, cp_doubles of room; part: csr_multi_stride(k) partial sums per segment, part_doubles of room.  Too little
// of either is RBL_ERR_STATE before anything is launched.  pack_done (optional) is recorded behind the interleaving.
int csr_multi_stride(int k);   // 2 for k <= 2, else 4
int launch_csr_gemvt_multi(const CsrStore* st, int64_t n, int64_t ld, int k, const double* const* c, double* Cp, size_t cp_doubles,
                           double* part, size_t part_doubles, double* const* q, int num_cu, hipStream_t s,
                           hipEvent_t pack_done = nullptr);
// rows [row0, row0 + rows) as dense fp64 rows of stride ldo (implicit entries +0.0)
int launch_csr_dense(const CsrStore* st, int64_t row0, int64_t rows, int64_t ldo, double* out, int num_cu, hipStream_t s);
// G = D^T D by one of two routes (route: 0 = the rule csr_gram_route of csr_gram_plan.h on st->pair_products, 2, 3);
// returns with s idle and everything transient freed; rep (optional): what ran, timed by HIP events.
// Route 2: chunks of csr_gram_chunk_rows(n, ld) rows expanded into a transient staging buffer (<= 256 MB), each through
// launch_gram(RBL_STORE_F64), added in chunk order.  Route 3 (spgram.hip): from the entries, tile_cols columns per
// accumulator tile (0 = the plan's); it needs the column form.
int64_t csr_gram_chunk_rows(int64_t n, int64_t ld);
int launch_csr_gram(const CsrStore* st, int64_t n, int64_t ld, int64_t d, double* slab, double* G, int num_cu, hipStream_t s,
                    int route = 0, int tile_cols = 0, rbl_gram_report* rep = nullptr);
int launch_csr_spgram(const CsrStore* st, int64_t n, int64_t ld, double* G, int num_cu, int tile_cols, hipStream_t s,
                      rbl_gram_report* rep);
unsigned spgram_grid(int64_t items, int num_cu);   // blocks of four single-wave items, at most 32 per CU

// ---- wstep_op.hip: the w-step of a handle without a Gram matrix (RBL_CREATE_NO_GRAM) ----------------------------
// A = rho D^T D + diag(.) applied through the two sparse passes.  What the operator needs beside the WstepWorkspace:
struct OpData {
    const CsrStore* st;    // the owner's entries, both forms
    int64_t n;
    double* t;             // n: t = D p
    double* slab;          // the segments' partial sums of y = D^T t, slab_doubles >= st->nseg of them
    size_t slab_doubles;
    double* part;          // op_part_doubles(ld): the chunks' partial sums and maxima of the d-space kernels
    int num_cu;            // sizes the grids of the sparse passes only; no bit of a result depends on it
};
size_t op_part_doubles(int64_t ld);
// launch_power_iteration through the operator: lambda_max(D^T D) after `iters` steps from the same start vector
int launch_op_power_iteration(const OpData& op, int64_t ld, int64_t d, double* x, double* y, double* scal, int iters,
                              double* lambda_host, hipStream_t s);
// ridge by CG, lasso / elastic net by FISTA (ws.pen_l1 / ws.pen_l2 as in run_wstep); ws.form = 4.  RBL_WSTEP_SMOOTH_L1
// is RBL_ERR_INVALID: its preconditioner is diag(G)
int run_wstep_op(int wstep, const OpData& op, int64_t ld, const double* q, double rho, double reg, double L, double tol,
                 int max_inner, double* w, WstepWorkspace& ws, int* iters_host, hipStream_t s);

// ---- wstep_ws.hip: the exact working-set lasso / elastic net on that route (RBL_CREATE_WORKING_SET) -----------------
// The working set of one handle (a borrower has its own).  plan is the host's bookkeeping (wset_plan.h), S / pos its
// device copies; Gs the WS_CAP-strided sub-Gram matrix; small the Gram-route workspace of the restricted problem.
struct WsetState {
    WsetPlan plan;
    DevArena* mem = nullptr;     // where the spare Gs of a compaction is allocated when an eviction first needs it
    double *Gs = nullptr, *Gs2 = nullptr;
    int *pos = nullptr, *S = nullptr, *keep = nullptr;
    double *qS = nullptr, *wS = nullptr, *l1S = nullptr, *l2S = nullptr;   // WS_CAP each
    double *vpart = nullptr, *qpart = nullptr;   // per chunk: largest violation outside S, max |q|
    int* ipart = nullptr;                        // ... and its column
    int* info = nullptr;                         // device: [0] coefficients != 0 after the last scatter
    int* pin = nullptr;                          // pinned: [0] sequence number (last), [1] columns chosen, [2] support, [3] candidate
                                                 // chunks, [4 ..] the columns
    int seq = 0;
    int num_cu = 256;            // caps k_ws_gram_rows' grid (one block per unit); no bit of Gs depends on it
    WstepWorkspace small{};
    int64_t epoch = -1;          // the data epoch Gs belongs to
    bool built = false;          // S / pos / Gs stand
    bool resync = true;          // w may have coefficients outside S (set from outside, or a w-step left the route)
    bool after_leave = false;    // ... the latter: w is what the operator FISTA left, and a support that still does not fit is
                                 // not worth a cold start
    void w_replaced() {          // w was written from outside the w-step (a state set, a w restored from w_prev)
        resync = true;
        after_leave = false;
    }
    int64_t bytes = 0;
    rbl_wset_report rep{};
};
// scan_only: what wset_scan uses alone (no Gs, no restricted-problem workspace)
int alloc_wset(DevArena& mem, WsetState& W, int64_t ld, hipStream_t s, bool scan_only = false);
// One w-step (RBL_WSTEP_L1).  cap: the slots S may use (WS_CAP; the test entry shrinks it).  l1_host: the handle's l1 on
// the host (d values) with per-coordinate penalties, for the free coordinates; ws.form = 5, or 4 when the w-step left
// the route (run_wstep_op's FISTA from the current w)
int run_wstep_ws(const OpData& op, int64_t ld, int64_t d, const double* q, double rho, double reg, double L, double tol,
                 int max_inner, double* w, WstepWorkspace& ws, WsetState& W, int cap, const double* l1_host, int* iters_host,
                 hipStream_t s);
// the pieces alone (rbl_k_wset_gram / rbl_k_wset_scan): append cols to S and form their rows of Gs; the scan's choice on a
// prescribed g (q may be NULL: zeros), kvec = kappa per column, member_pos = the host's pos (ld ints)
int wset_gram(const CsrStore* st, WsetState& W, int64_t ld, const int* cols, int n, int num_cu, hipStream_t s);
int wset_scan(WsetState& W, int64_t ld, int64_t d, const double* g, const double* q, const double* kvec, const int* member_pos,
              double tol, int take, int* count, int* cols, hipStream_t s);

// ---- synth.hip --------------------------------------------------------------------------
int launch_synth(int storage, void* D, int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed,
                 double class_sep, double flip_y, const int* special, const double* mix, const double* A16,
                 const int* vertex, signed char* ysign, hipStream_t s);
// RBL_STORE_F16 (the matrix is written once, from regenerated draws): the labels and the column sums / sums of squares
// of the unrounded fp32 draws (slab: 2 x synth_stats_rows(num_cu) x ld doubles), then D = half(-y (x - mean) inv_std)
int synth_stats_rows(int num_cu);
int launch_synth_stats(int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed, double class_sep, double flip_y,
                       const int* special, const double* mix, const double* A16, const int* vertex, signed char* ysign,
                       double* slab, double* sum, double* sumsq, int num_cu, hipStream_t s);
int launch_synth_f16(void* D, int64_t n, int64_t ld, int64_t d, int64_t row_offset, u64 seed, double class_sep, double flip_y,
                     const int* special, const double* mix, const double* A16, const int* vertex, const double* mean,
                     const double* inv_std, hipStream_t s);

// ---- zband.hip: z-step for piecewise-constant rank weights without a sort -------------------
constexpr int ZB_BITS = 11;          // radix-select digit (last pass: the remaining 9 bits)
constexpr int ZB_C = 16;             // candidate block values per root pass
constexpr int ZB_ROOT_PASSES = 4;    // bracket shrinks 15x per pass (the first one far more when the prediction is good)
constexpr int ZB_GCAP = 2048;        // undecided elements the finishing kernel settles exactly
constexpr int ZB_MAX_BANDS = 8;
constexpr int ZB_MAX_TARGETS = 12;
constexpr int ZB_MAX_GROUPS = 6;     // distinct key prefixes among the targets in one select pass
constexpr int ZB_MAX_CLUSTERS = 4;
enum { ZB_OK = 0, ZB_TIE = 1, ZB_BAD = 2, ZB_GROUPS = 3, ZB_BRACKET = 4, ZB_UNRESOLVED = 5, ZB_SWALLOW_L = 6, ZB_SWALLOW_R = 7,
       ZB_ONESIDED = 8, ZB_OVERLAP = 9 };

struct ZbConfig {                        // built once from sigma (host), passed to the kernels by value
    int nbands;
    long long start[ZB_MAX_BANDS + 1];   // first rank of band j; start[nbands] = n
    double sigma[ZB_MAX_BANDS];
    int ntargets;
    long long target_rank[ZB_MAX_TARGETS];   // ascending, unique
    int last_t[ZB_MAX_BANDS];            // target index of band j's last rank  (j < nbands - 1)
    int first_t[ZB_MAX_BANDS];           // target index of band j's first rank (j > 0)
    int nclusters;                       // edge clusters: band L | single-rank bands | band R
    int cl_L[ZB_MAX_CLUSTERS], cl_R[ZB_MAX_CLUSTERS];
    int cl_root[ZB_MAX_CLUSTERS];        // sigma increases somewhere along the chain: pooling is possible
};
struct ZbState {                         // device scratch of one z-step
    u64 prefix[ZB_MAX_TARGETS];
    long long rem[ZB_MAX_TARGETS];
    int group[ZB_MAX_TARGETS];
    u64 gprefix[ZB_MAX_TARGETS];
    u64 key[ZB_MAX_TARGETS];
    long long eq[ZB_MAX_TARGETS];         // keys equal to key[t] (rem[t] ends as the target's rank among them)
    int ngroups;
    int status;
    double cand[ZB_MAX_CLUSTERS][ZB_C];
    int done[ZB_MAX_CLUSTERS];
    int has_block[ZB_MAX_CLUSTERS];
    double x[ZB_MAX_CLUSTERS];
    double xh[ZB_MAX_CLUSTERS][3];        // block values of the last three certified iterations (kept across z-steps)
    int nh[ZB_MAX_CLUSTERS];
    double br[ZB_MAX_CLUSTERS][2];        // bracket of the root after the last pass
    double frozen[ZB_MAX_CLUSTERS][4];    // outside the bracket for certain: top count / sum m, bottom count / sum m
    double und[ZB_MAX_CLUSTERS];          // elements whose membership changes inside the bracket
    int gcount[ZB_MAX_CLUSTERS];          // gathered so far
    double blk[ZB_MAX_CLUSTERS][2];       // the certified block: elements of band L / of band R in it
    int canon[ZB_MAX_CLUSTERS];           // x[k] comes from sums over the certified block alone (k_zb_canon), or is an exact -1
};
size_t zb_hist_bytes();
size_t zb_partials_bytes();
int launch_zb_edges(const double* sigma, int64_t n, long long* pos, int* counter, int cap, hipStream_t s);
// z = the z-step, c = z + lambda/rho in the same pass
// rs (optional): z and c are written in the owner's sign convention (z~ = r z, c~ = z~ + lambda~/rho); keys and m are the true m's
int launch_zband(int loss, const ZbConfig& cfg, int64_t n, double rho, const u64* keys, const double* m, double* z,
                 const double* lam, double* c, ZbState* st, u32* hist, double* partials, int* pin, int seq, u32* counters, hipStream_t s,
                 const signed char* rs = nullptr);
int launch_zband_risk(int loss, const ZbConfig& cfg, int64_t n, const u64* keys, ZbState* st, u32* hist, double* partials,
                      double* out_dev, hipStream_t s);
// the steps of launch_zband one by one (multi-GPU driver: collectives in between)
int launch_zbd_init(const ZbConfig& cfg, ZbState* st, u32* hist, hipStream_t s);
int launch_zbd_hist(int64_t n, const u64* keys, ZbState* st, u32* hist, int pass, hipStream_t s);
int launch_zbd_scan(int loss, const ZbConfig& cfg, ZbState* st, u32* hist, int pass, double rho, hipStream_t s);
int launch_zbd_eval(int loss, const ZbConfig& cfg, int64_t n, const u64* keys, ZbState* st, int k, double rho, double* partials,
                    double* tot, hipStream_t s);
int launch_zbd_decide(int loss, const ZbConfig& cfg, ZbState* st, int k, double rho, const double* tot, int last, hipStream_t s,
                      int* pin_settled = nullptr, int dseq = 0);
int launch_zbd_gather(int loss, const ZbConfig& cfg, int64_t n, const u64* keys, ZbState* st, int k, double rho, double* partials,
                      double* pack, hipStream_t s);
int launch_zbd_finish(int loss, const ZbConfig& cfg, ZbState* st, int k, double rho, double* partials, const double* packs_all,
                      int world, hipStream_t s);
int launch_zbd_apply(int loss, const ZbConfig& cfg, int64_t n, double rho, const double* m, double* z, const double* lam, double* c,
                     ZbState* st, int* pin, int seq, u32* counters, hipStream_t s);
