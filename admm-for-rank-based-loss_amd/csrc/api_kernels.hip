// api_kernels.hip - the kernel-level entry points (rbl_k_*) of the parity tests: host buffers in, host buffers out.
#include "api_internal.h"
#include "csr_plan.h"
#include "csr_gram_plan.h"

// =================================================== kernel-level entry points (host buffers)
// They run on the same workspace allocators as the solver handle (alloc_sort, alloc_pav, alloc_prefix, alloc_wstep).
namespace {
struct Scratch {   // the buffers and the stream of one call
    DevArena mem;
    hipStream_t s = nullptr;
    ~Scratch() {
        if (s) (void)hipStreamDestroy(s);
    }
    template <typename T>
    int upload(T** p, const T* host, size_t count) {
        RBL_TRY(mem.alloc(p, count));
        if (count) RBL_HIP(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
        return RBL_OK;
    }
};

int scratch_begin(Scratch& sc, int* num_cu) {
    RBL_TRY(check_device(nullptr));
    RBL_HIP(hipStreamCreateWithFlags(&sc.s, hipStreamNonBlocking));
    if (num_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        RBL_HIP(hipGetDevice(&dev));
        RBL_HIP(hipGetDeviceProperties(&prop, dev));
        *num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return RBL_OK;
}

// D (host fp64 n x d) -> device storage with ld padding
int upload_matrix(Scratch& sc, int storage, int64_t n, int64_t d, const double* D, void** Dd, int64_t* ld_out) {
    if (storage != RBL_STORE_F32 && storage != RBL_STORE_F64 && storage != RBL_STORE_F16) {   // (sparse: the rbl_k_csr_* entries)
        rbl_set_error("kernel-level entry: storage must be RBL_STORE_F32, RBL_STORE_F64 or RBL_STORE_F16 (got %d)", storage);
        return RBL_ERR_INVALID;
    }
    const int64_t ld = rbl_storage_ld(storage, d);
    const size_t esz = rbl_storage_esz(storage);
    std::vector<unsigned char> host((size_t)n * ld * esz, 0);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t j = 0; j < d; ++j) {
            if (storage == RBL_STORE_F16) ((unsigned short*)host.data())[r * ld + j] = f64_to_f16_bits(D[r * d + j]);
            else if (storage == RBL_STORE_F32) ((float*)host.data())[r * ld + j] = (float)D[r * d + j];
            else ((double*)host.data())[r * ld + j] = D[r * d + j];
        }
    RBL_TRY(sc.upload((unsigned char**)Dd, host.data(), host.size()));
    *ld_out = ld;
    return RBL_OK;
}

// A host CSR matrix that holds D itself -> a CsrStore in the call's arena, through the launches rbl_set_data_csr runs on a
// handle with RBL_STORE_CSR: the forming kernel (labels -1, so -y x = x; one chunk), then the lane group and, with
// `columns`, the column form and its segment table.
int upload_csr(Scratch& sc, const char* who, int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
               bool columns, int num_cu, CsrStore* st, int64_t* ld_out) {
    if (n < 1 || n > 0x7fffffffLL || d < 1 || !indptr) {
        rbl_set_error("%s: 1 <= n <= 2^31 - 1, d >= 1 and indptr are needed (n = %lld, d = %lld)", who, (long long)n, (long long)d);
        return RBL_ERR_INVALID;
    }
    int64_t row = 0, got = 0;
    const int64_t nnz = indptr[n];
    if (nnz < 0 || nnz > 0x7fffffffLL || csr_check_indptr(indptr, n, nnz, &row, &got) != CSR_PLAN_OK || (nnz > 0 && (!indices || !values))) {
        rbl_set_error("%s: indptr must start at 0, not decrease and end at nnz <= 2^31 - 1 (indices / values given)", who);
        return RBL_ERR_INVALID;
    }
    const int64_t ld = rbl_storage_ld(RBL_STORE_CSR, d);
    memset(st, 0, sizeof(CsrStore));
    RBL_TRY(csr_store_reserve(sc.mem, st, n, ld, nnz, columns));
    st->pair_products = csr_gram_pair_products(indptr, n, 0);
    RBL_HIP(hipMemcpy(st->indptr, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
    int32_t* di = nullptr;
    double* dv = nullptr;
    signed char* ys = nullptr;
    u64* err = nullptr;
    RBL_TRY(sc.upload(&di, indices, (size_t)nnz));
    RBL_TRY(sc.upload(&dv, values, (size_t)nnz));
    RBL_TRY(sc.mem.alloc(&ys, (size_t)n));
    RBL_TRY(sc.mem.alloc(&err, 2));
    const u64 pair0[2] = {0ull, ~0ull};
    RBL_HIP(hipMemcpy(err, pair0, sizeof(pair0), hipMemcpyHostToDevice));
    RBL_HIP(hipMemsetAsync(ys, 0xff, (size_t)n, sc.s));   // y = -1
    RBL_TRY(launch_csr_store(RBL_DTYPE_F64, RBL_INDEX_I32, st, n, 0, d, 0, di, dv, 0, nnz, ys, err, num_cu, sc.s));
    u64 bad[2] = {0ull, 0ull};
    RBL_HIP(hipMemcpyAsync(bad, err, sizeof(bad), hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (bad[0] > 0) {
        rbl_set_error("%s: %llu entries refused, first in row %llu - the columns of a row must lie in [0, d) and increase strictly",
                      who, bad[0], bad[1]);
        return RBL_ERR_INVALID;
    }
    RBL_TRY(csr_store_finish(st, ld, columns, num_cu, sc.s));
    *ld_out = ld;
    return RBL_OK;
}
}  // namespace

extern "C" {

// the kernel-level entry points check the loss id before any device work
static int k_check_loss(const char* who, int loss) {
    if (rbl_check_loss(loss) == RBL_OK) return RBL_OK;
    rbl_set_error("%s: unknown loss id %d", who, loss);
    return RBL_ERR_INVALID;
}

int rbl_k_prox(int loss, int64_t n, const double* sigma, double rho, const double* m, double* out) {
    RBL_TRY(k_check_loss("rbl_k_prox", loss));
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0) return RBL_OK;
    double *ds = nullptr, *dm = nullptr, *dout = nullptr;
    RBL_TRY(sc.upload(&ds, sigma, (size_t)n));
    RBL_TRY(sc.upload(&dm, m, (size_t)n));
    RBL_TRY(sc.mem.alloc(&dout, (size_t)n));
    RBL_TRY(launch_prox(loss, n, ds, rho, dm, dout, sc.s));
    RBL_HIP(hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_sort(int64_t n, const double* keys, double* sorted_keys, uint32_t* perm) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0) return RBL_OK;
    double *dk = nullptr, *ms = nullptr;
    RBL_TRY(sc.upload(&dk, keys, (size_t)n));
    SortWorkspace sw{};
    RBL_TRY(alloc_sort(sc.mem, sw, n, true, sc.s));
    RBL_TRY(sc.mem.alloc(&ms, (size_t)n));
    RBL_TRY(launch_keys_from_m(n, dk, sw.keys[0], sw.vals[0], sc.s));
    RBL_TRY(launch_radix_sort(sw, n, true, sc.s));
    RBL_TRY(launch_unflip_keys(n, sw.keys[0], ms, sc.s));
    if (sorted_keys) RBL_HIP(hipMemcpyAsync(sorted_keys, ms, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    if (perm) RBL_HIP(hipMemcpyAsync(perm, sw.vals[0], sizeof(u32) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

// The sort of the z-step with 32-bit keys: the launches of z_step_sorted's use32 branch, in its order, on buffers laid
// out as a handle's (rbl_phase_m: launch_make_m_range with v = m, lambda = 0, rho = 1 - m - 0/1 has the input's bits).
// The fix-up compares m numerically: -0.0 and +0.0 tie and keep their row order, where rbl_k_sort orders the bit
// patterns (every -0.0 before every +0.0).  *flag = 1: a run of more than S32_MAX_RUN equal keys; m_sorted / ids are
// then meaningless (zb_resolve redoes such a z-step with 64-bit keys).
int rbl_k_sort32(int64_t n, const double* m, uint32_t idx_off, double* m_sorted, uint32_t* ids, int* flag) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (flag) *flag = 0;
    if (n <= 0) return RBL_OK;
    if (!m || n + (int64_t)idx_off > (1LL << 32)) {
        rbl_set_error("rbl_k_sort32: m is NULL or n + idx_off exceeds 2^32 (row ids are 32 bits)");
        return RBL_ERR_INVALID;
    }
    double *dv = nullptr, *dlam = nullptr, *dm = nullptr, *ms = nullptr;
    u64* mm = nullptr;
    int* dflag = nullptr;
    RBL_TRY(sc.upload(&dv, m, (size_t)n));
    RBL_TRY(sc.mem.alloc(&dlam, (size_t)n));
    RBL_TRY(sc.mem.alloc(&dm, (size_t)n));
    RBL_TRY(sc.mem.alloc(&ms, (size_t)n));
    RBL_TRY(sc.mem.alloc(&mm, (size_t)s32_range_words()));
    RBL_TRY(sc.mem.alloc(&dflag, 1));
    RBL_HIP(hipMemsetAsync(dlam, 0, sizeof(double) * n, sc.s));
    SortWorkspace sw{};
    RBL_TRY(alloc_sort(sc.mem, sw, n, true, sc.s));
    u32* k32 = reinterpret_cast<u32*>(sw.keys[0]);
    RBL_TRY(launch_make_m_range(n, 1.0, dv, dlam, dm, mm, sc.s, nullptr));
    RBL_TRY(launch_keys32(n, dm, mm, k32, sw.vals[0], idx_off, sc.s));
    RBL_TRY(launch_radix_sort32(sw, n, sc.s));
    RBL_TRY(launch_sort32_fix(n, k32, sw.vals[0], dm, idx_off, ms, sw.vals[1], dflag, sc.s));
    if (m_sorted) RBL_HIP(hipMemcpyAsync(m_sorted, ms, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    if (ids) RBL_HIP(hipMemcpyAsync(ids, sw.vals[1], sizeof(u32) * n, hipMemcpyDeviceToHost, sc.s));
    int f = 0;
    RBL_HIP(hipMemcpyAsync(&f, dflag, sizeof(int), hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (flag) *flag = f;
    return RBL_OK;
}

// ncalls successive PAV solves on ONE workspace (m_sorted: ncalls x n): the hints of the upper seams, the barrier parity
// and the EHRM speculated branch carry over from one call to the next as they do between the z-steps of a solve.
static int k_pav_common(int loss, int64_t n, const double* sigma_a, const double* sigma_b, int ehrm, double B,
                        double rho, int ncalls, const double* m_sorted, int branch_in, int upper, double* out,
                        int64_t* n_merges, int* branch_out, uint32_t* counters_out) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (n <= 0 || ncalls <= 0) return RBL_OK;
    double *sa = nullptr, *sb = nullptr;
    RBL_TRY(sc.upload(&sa, sigma_a, (size_t)n));
    if (ehrm) RBL_TRY(sc.upload(&sb, sigma_b, (size_t)n));
    else sb = sa;
    PavWorkspace pw{};   // the sorted m goes to pw.ms, its prefix sums to pw.pm
    RBL_TRY(alloc_pav(sc.mem, pw, n, sc.s));
    PrefixBufs pa, pb;
    RBL_TRY(alloc_prefix(sc.mem, pa, n));
    pb = pa;
    if (ehrm) RBL_TRY(alloc_prefix(sc.mem, pb, n));
    PavExtras ex = pw.ex;
    {
        int dev = 0, cus = 0;
        RBL_HIP(hipGetDevice(&dev));
        RBL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        ex.num_cu = cus;
    }
    ex.B = B;
    ex.upper = upper;
    {
        const char* e = getenv("RBL_EHRM_SPEC");   // 0 / 1: the speculated branch; -1: round 2's separate pass
        if (e && (atoi(e) == 0 || atoi(e) == 1)) ex.spec = atoi(e);
        // a forced branch (the tests pin both) and RBL_EHRM_SPEC=-1 go through the separate test; the automatic choice
        // through the speculation inside the bottom kernel
        if (!ehrm || branch_in >= 0 || (e && atoi(e) == -1)) ex.fpart = nullptr;
    }
    RBL_TRY(launch_prefix(sa, n, pa, sc.s));
    if (ehrm) RBL_TRY(launch_prefix(sb, n, pb, sc.s));
    // identity permutation scatter applies the EHRM clip
    std::vector<u32> idh((size_t)n);
    for (int64_t i = 0; i < n; ++i) idh[(size_t)i] = (u32)i;
    u32* idd = nullptr;
    double* zz = nullptr;
    RBL_TRY(sc.upload(&idd, idh.data(), (size_t)n));
    RBL_TRY(sc.mem.alloc(&zz, (size_t)n));
    for (int call = 0; call < ncalls; ++call) {
        RBL_HIP(hipMemcpyAsync(pw.ms, m_sorted + (size_t)call * n, sizeof(double) * n, hipMemcpyHostToDevice, sc.s));
        RBL_TRY(launch_prefix(pw.ms, n, pw.pm, sc.s));
        if (ehrm && !ex.fpart) RBL_TRY(launch_ehrm_branch(n, sa, sb, B, rho, pw.ms, pw.partials, pw.branch, branch_in, sc.s));
        RBL_TRY(launch_pav_tree(loss, n, rho, pw.ms, sa, sb, pw.u, pa.view(), pb.view(), pw.pm.view(), ehrm ? pw.branch : nullptr,
                                pw.recs, pw.counters, sc.s, nullptr, nullptr, &ex));
        RBL_TRY(launch_scatter_z(n, pw.u, idd, ehrm ? pw.branch : nullptr, B, ehrm, rho, nullptr, zz, nullptr, 0, n, sc.s));
        RBL_HIP(hipMemcpyAsync(out + (size_t)call * n, zz, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
        unsigned mc4[4] = {0, 0, 0, 0};
        int br = -1;
        RBL_HIP(hipMemcpyAsync(mc4, pw.counters, sizeof(mc4), hipMemcpyDeviceToHost, sc.s));
        if (ehrm) RBL_HIP(hipMemcpyAsync(&br, pw.branch, sizeof(int), hipMemcpyDeviceToHost, sc.s));
        RBL_HIP(hipStreamSynchronize(sc.s));
        if (counters_out)
            for (int j = 0; j < 4; ++j) counters_out[4 * call + j] = mc4[j];
        if (mc4[3] != 0) {
            rbl_set_error("PAV: the upper-level kernel did not complete (a wait gave up or its fill list overflowed)");
            return RBL_ERR_HIP;
        }
        if (n_merges) n_merges[call] = mc4[0];
        if (branch_out) branch_out[call] = br;
        if (ehrm && br >= 0) ex.spec = br;   // the next call speculates the branch this one took (rbl_phase_finish)
    }
    return RBL_OK;
}

int rbl_k_pav(int loss, int64_t n, const double* sigma, double rho, const double* m_sorted, double* out,
              int64_t* n_merges) {
    RBL_TRY(k_check_loss("rbl_k_pav", loss));
    return k_pav_common(loss, n, sigma, sigma, 0, 0.0, rho, 1, m_sorted, -1, PAV_UPPER_DEFAULT, out, n_merges, nullptr,
                        nullptr);
}

int rbl_k_pav_ehrm(int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho,
                   const double* m_sorted, int branch, double* out, int* branch_out) {
    return k_pav_common(RBL_LOSS_BCE, n, sigma_a, sigma_b, 1, B, rho, 1, m_sorted, branch, PAV_UPPER_DEFAULT, out, nullptr,
                        branch_out, nullptr);
}

int rbl_k_pav_seq(int loss, int64_t n, const double* sigma_a, const double* sigma_b, double B, double rho, int ncalls,
                  const double* m_sorted, int upper, double* out, int* branch_out, uint32_t* counters) {
    RBL_TRY(k_check_loss("rbl_k_pav_seq", loss));
    if (upper != RBL_PAV_UPPER_PERSIST && upper != RBL_PAV_UPPER_TWO_LAUNCH) {
        rbl_set_error("rbl_k_pav_seq: upper must be RBL_PAV_UPPER_PERSIST or RBL_PAV_UPPER_TWO_LAUNCH, got %d", upper);
        return RBL_ERR_INVALID;
    }
    const int ehrm = sigma_b != nullptr;
    if (ehrm && loss != RBL_LOSS_BCE) {
        rbl_set_error("rbl_k_pav_seq: the EHRM z-step is defined for the BCE loss only");
        return RBL_ERR_INVALID;
    }
    return k_pav_common(loss, n, sigma_a, ehrm ? sigma_b : sigma_a, ehrm, B, rho, ncalls, m_sorted, -1,
                        upper == RBL_PAV_UPPER_PERSIST ? PAV_UPPER_PERSIST : PAV_UPPER_TWO_LAUNCH, out, nullptr, branch_out,
                        counters);
}

int rbl_k_gemv(int storage, int64_t n, int64_t d, const double* D, const double* w, double* v) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    if (n <= 0) return RBL_OK;
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    std::vector<double> wp((size_t)ld, 0.0);
    for (int64_t j = 0; j < d; ++j) wp[(size_t)j] = w[j];
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(sc.upload(&dw, wp.data(), (size_t)ld));
    RBL_TRY(sc.mem.alloc(&dv, (size_t)n));
    RBL_TRY(launch_gemv(storage, Dd, n, ld, dw, dv, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(v, dv, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemvt(int storage, int64_t n, int64_t d, const double* D, const double* c, double* q) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n > 0 ? n : 0, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, c, (size_t)n));
    RBL_TRY(sc.mem.alloc(&slab, (size_t)gemvt_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_TRY(launch_gemvt(storage, Dd, n, ld, dc, slab, dq, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(q, dq, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemv_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* W, double* V) {
    if (k < 1 || k > 64 || d <= 0) {
        rbl_set_error("rbl_k_gemv_multi: 1..64 columns, d > 0");
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    if (n <= 0) return RBL_OK;
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    std::vector<double> wp((size_t)ld * k, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < d; ++i) wp[(size_t)j * ld + i] = W[(size_t)j * d + i];
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(sc.upload(&dw, wp.data(), wp.size()));
    RBL_TRY(sc.mem.alloc(&dv, (size_t)n * k));
    const bool multi = sweep_multi_supported(storage, ld);
    const int kpp = multi ? sweep_multi_k(storage, ld) : 1;
    for (int j0 = 0; j0 < k; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {   // outside the multi-column kernels' widths: the single-column pass per column
            RBL_TRY(launch_gemv(storage, Dd, n, ld, dw + (size_t)j0 * ld, dv + (size_t)j0 * n, num_cu, sc.s));
            continue;
        }
        const double* w[RBL_MULTI_KMAX];
        double* v[RBL_MULTI_KMAX];
        for (int j = 0; j < kk; ++j) {
            w[j] = dw + (size_t)(j0 + j) * ld;
            v[j] = dv + (size_t)(j0 + j) * n;
        }
        RBL_TRY(launch_sweep_v_multi(storage, Dd, n, ld, kk, w, nullptr, nullptr, v, nullptr, nullptr, nullptr, num_cu, sc.s));
    }
    RBL_HIP(hipMemcpyAsync(V, dv, sizeof(double) * n * k, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_gemvt_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* Cm, double* Q) {
    if (k < 1 || k > 64 || d <= 0) {
        rbl_set_error("rbl_k_gemvt_multi: 1..64 columns, d > 0");
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n > 0 ? n : 0, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, Cm, (size_t)(n > 0 ? n : 0) * k));
    const bool multi = n > 0 && sweep_multi_supported(storage, ld);
    const int kpp = multi ? sweep_multi_k(storage, ld) : 1;
    RBL_TRY(sc.mem.alloc(&slab, multi ? sweep_multi_slab_doubles(ld, num_cu) : (size_t)gemvt_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld * k));
    for (int j0 = 0; j0 < k; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {
            RBL_TRY(launch_gemvt(storage, Dd, n, ld, dc + (size_t)j0 * (n > 0 ? n : 0), slab, dq + (size_t)j0 * ld, num_cu, sc.s));
            continue;
        }
        const double* c[RBL_MULTI_KMAX];
        double* q[RBL_MULTI_KMAX];
        for (int j = 0; j < kk; ++j) {
            c[j] = dc + (size_t)(j0 + j) * n;
            q[j] = dq + (size_t)(j0 + j) * ld;
        }
        RBL_TRY(launch_sweep_q_multi(storage, Dd, n, ld, kk, c, slab, q, num_cu, sc.s));
    }
    for (int j = 0; j < k; ++j)
        RBL_HIP(hipMemcpyAsync(Q + (size_t)j * d, dq + (size_t)j * ld, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

// ---- the row-streaming passes on prescribed inputs with a caller-chosen grid (rbl_k_sweep_*): the launchers of a solve,
// unchanged, with num_cu in the place of the device's CU count; buffers sized by the launchers' own rules for that num_cu
namespace {
constexpr int SWEEP_GUARD = 64;   // doubles behind row n of every row-wise array, preset like the rows

// the checks that come before any device work; ld of the stored matrix
int sweep_begin(Scratch& sc, const char* who, int storage, int64_t n, int64_t d, int num_cu, int64_t* ld) {
    if (storage != RBL_STORE_F32 && storage != RBL_STORE_F64 && storage != RBL_STORE_F16) {
        rbl_set_error("%s: storage must be RBL_STORE_F32, RBL_STORE_F64 or RBL_STORE_F16 (got %d)", who, storage);
        return RBL_ERR_INVALID;
    }
    if (n < 1 || d < 1) {
        rbl_set_error("%s: n >= 1 and d >= 1 are needed (n = %lld, d = %lld)", who, (long long)n, (long long)d);
        return RBL_ERR_INVALID;
    }
    int cus = 0;
    RBL_TRY(scratch_begin(sc, &cus));
    if (num_cu < 1 || num_cu > cus) {
        rbl_set_error("%s: num_cu = %d outside 1..%d (the device's compute units)", who, num_cu, cus);
        return RBL_ERR_INVALID;
    }
    *ld = rbl_storage_ld(storage, d);
    return RBL_OK;
}

// rows x (n + SWEEP_GUARD) doubles on the device, every byte 0xff (a NaN); init (rows_init x n, host) fills the first rows
int rows_alloc(Scratch& sc, double** p, int64_t n, int rows, const double* init, int rows_init) {
    const size_t stride = (size_t)n + SWEEP_GUARD;
    std::vector<double> host(stride * rows);
    memset(host.data(), 0xff, host.size() * sizeof(double));
    for (int r = 0; r < rows_init; ++r) memcpy(host.data() + r * stride, init + (size_t)r * n, sizeof(double) * (size_t)n);
    return sc.upload(p, host.data(), host.size());
}

// back to the host (out: rows x n, may be NULL); a guard that no longer holds 0xff is a write past row n
int rows_fetch(Scratch& sc, const char* who, const char* what, const double* p, int64_t n, int rows, double* out) {
    const size_t stride = (size_t)n + SWEEP_GUARD;
    std::vector<double> host(stride * rows);
    RBL_HIP(hipMemcpyAsync(host.data(), p, host.size() * sizeof(double), hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int r = 0; r < rows; ++r) {
        const unsigned char* g = (const unsigned char*)(host.data() + r * stride + n);
        for (size_t b = 0; b < SWEEP_GUARD * sizeof(double); ++b)
            if (g[b] != 0xff) {
                rbl_set_error("%s: %s (column %d) was written past row n = %lld", who, what, r, (long long)n);
                return RBL_ERR_STATE;
            }
        if (out) memcpy(out + (size_t)r * n, host.data() + r * stride, sizeof(double) * (size_t)n);
    }
    return RBL_OK;
}

// vectors over the columns (k x d, host) padded to k x ld on the device
int cols_upload(Scratch& sc, double** p, const double* host, int k, int64_t d, int64_t ld) {
    std::vector<double> wp((size_t)ld * k, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < d; ++i) wp[(size_t)j * ld + i] = host[(size_t)j * d + i];
    return sc.upload(p, wp.data(), wp.size());
}

void instance_out(int* instance, const SweepInstance& in) {
    if (!instance) return;
    instance[0] = in.kind;
    instance[1] = in.p;
    instance[2] = in.r;
    instance[3] = in.s;
    instance[4] = in.blocks;
}
}  // namespace

// rbl_k_sweep_erm (sigma == NULL) and rbl_k_sweep_erm_w (sigma: n host doubles, one per row): one body, the same presets,
// guards and reporting
static int k_sweep_erm_any(const char* who, int storage, int loss, int64_t n, int64_t d, const double* D, const double* w,
                           const double* z_old, const double* lam, double sigma0, const double* sigma, double rho,
                           double rho_next, int num_cu, int want_v, double* lam_out, double* v, double* z_new, double* q,
                           double* primal2, double* zz, int* instance) {
    RBL_TRY(k_check_loss(who, loss));
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (!sweep_erm_supported(storage, ld)) {
        rbl_set_error("%s: d = %lld (ld = %lld) is outside the single-sweep kernels' widths for this storage", who, (long long)d,
                      (long long)ld);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dw = nullptr, *dz = nullptr, *dlam = nullptr, *dv = nullptr, *dzn = nullptr, *pred = nullptr, *slab = nullptr,
           *partials = nullptr, *dq = nullptr, *red = nullptr;
    RBL_TRY(cols_upload(sc, &dw, w, 1, d, ld));
    RBL_TRY(sc.upload(&dz, z_old, (size_t)n));
    RBL_TRY(rows_alloc(sc, &dlam, n, 1, lam, 1));
    RBL_TRY(rows_alloc(sc, &dv, n, 1, nullptr, 0));
    RBL_TRY(rows_alloc(sc, &dzn, n, 1, nullptr, 0));
    const double pred_h[2] = {rho_next, 0.0};
    RBL_TRY(sc.upload(&pred, pred_h, 2));
    RBL_TRY(sc.mem.alloc(&slab, (size_t)sweep_erm_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&partials, std::max((size_t)sweep_erm_blocks(num_cu) * 3, (size_t)reduce_blocks() * 4)));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_TRY(sc.mem.alloc(&red, 8));
    double* dsig = nullptr;
    if (sigma) RBL_TRY(sc.upload(&dsig, sigma, (size_t)n));
    SweepInstance inst{};
    RBL_TRY(launch_sweep_erm(storage, loss, Dd, n, ld, dw, dz, dlam, dv, dzn, sigma0, rho, pred, slab, partials, dq, red, red + 4,
                             num_cu, sc.s, nullptr, want_v ? 1 : 0, &inst, dsig));
    RBL_TRY(rows_fetch(sc, who, "lambda", dlam, n, 1, lam_out));
    RBL_TRY(rows_fetch(sc, who, "v", dv, n, 1, v));
    RBL_TRY(rows_fetch(sc, who, "z_new", dzn, n, 1, z_new));
    double redh[8];
    RBL_HIP(hipMemcpyAsync(q, dq, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipMemcpyAsync(redh, red, sizeof(redh), hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (primal2) *primal2 = redh[0];
    if (zz) *zz = redh[4];
    instance_out(instance, inst);
    return RBL_OK;
}

int rbl_k_sweep_erm(int storage, int loss, int64_t n, int64_t d, const double* D, const double* w, const double* z_old,
                    const double* lam, double sigma0, double rho, double rho_next, int num_cu, int want_v, double* lam_out,
                    double* v, double* z_new, double* q, double* primal2, double* zz, int* instance) {
    return k_sweep_erm_any("rbl_k_sweep_erm", storage, loss, n, d, D, w, z_old, lam, sigma0, nullptr, rho, rho_next, num_cu,
                           want_v, lam_out, v, z_new, q, primal2, zz, instance);
}

int rbl_k_sweep_erm_w(int storage, int loss, int64_t n, int64_t d, const double* D, const double* w, const double* z_old,
                      const double* lam, const double* sigma, double rho, double rho_next, int num_cu, int want_v,
                      double* lam_out, double* v, double* z_new, double* q, double* primal2, double* zz, int* instance) {
    if (!sigma) {
        rbl_set_error("rbl_k_sweep_erm_w: sigma is NULL");
        return RBL_ERR_INVALID;
    }
    return k_sweep_erm_any("rbl_k_sweep_erm_w", storage, loss, n, d, D, w, z_old, lam, 0.0, sigma, rho, rho_next, num_cu, want_v,
                           lam_out, v, z_new, q, primal2, zz, instance);
}

int rbl_k_sweep_v(int storage, int64_t n, int64_t d, const double* D, const double* w, const double* z, const double* lam,
                  double rho, int num_cu, double* lam_out, double* v, double* primal2, int* instance) {
    const char* who = "rbl_k_sweep_v";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (!sweep_v_supported(storage, ld)) {
        rbl_set_error("%s: d = %lld (ld = %lld) is outside the V-only pass' widths for this storage", who, (long long)d, (long long)ld);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dw = nullptr, *dz = nullptr, *dlam = nullptr, *dv = nullptr, *partials = nullptr, *red = nullptr;
    RBL_TRY(cols_upload(sc, &dw, w, 1, d, ld));
    RBL_TRY(sc.upload(&dz, z, (size_t)n));
    RBL_TRY(rows_alloc(sc, &dlam, n, 1, lam, 1));
    RBL_TRY(rows_alloc(sc, &dv, n, 1, nullptr, 0));
    RBL_TRY(sc.mem.alloc(&partials, (size_t)num_cu * 3));
    RBL_TRY(sc.mem.alloc(&red, 8));
    SweepInstance inst{};
    RBL_TRY(launch_sweep_v(storage, Dd, n, ld, dw, dz, dlam, dv, rho, partials, red, num_cu, sc.s, nullptr, &inst));
    RBL_TRY(rows_fetch(sc, who, "lambda", dlam, n, 1, lam_out));
    RBL_TRY(rows_fetch(sc, who, "v", dv, n, 1, v));
    double redh[2];
    RBL_HIP(hipMemcpyAsync(redh, red, sizeof(redh), hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (primal2) *primal2 = redh[0];
    instance_out(instance, inst);
    return RBL_OK;
}

int rbl_k_sweep_q(int storage, int64_t n, int64_t d, const double* D, const double* c, int num_cu, double* q, int* instance) {
    const char* who = "rbl_k_sweep_q";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (!sweep_v_supported(storage, ld)) {
        rbl_set_error("%s: d = %lld (ld = %lld) is outside the Q-only pass' widths for this storage", who, (long long)d, (long long)ld);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, c, (size_t)n));
    RBL_TRY(sc.mem.alloc(&slab, (size_t)sweep_erm_slab_rows(num_cu) * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    SweepInstance inst{};
    RBL_TRY(launch_sweep_q(storage, Dd, n, ld, dc, slab, dq, num_cu, sc.s, nullptr, &inst));
    RBL_HIP(hipMemcpyAsync(q, dq, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    instance_out(instance, inst);
    return RBL_OK;
}

int rbl_k_sweep_v_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* W, const double* Z,
                        const double* LAM, const double* rho, int num_cu, double* LAM_out, double* V, double* primal2,
                        int* instance) {
    const char* who = "rbl_k_sweep_v_multi";
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("%s: %d columns (1..%d)", who, k, RBL_MULTI_KMAX);
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (!sweep_multi_supported(storage, ld)) {
        rbl_set_error("%s: d = %lld (ld = %lld) is outside the multi-column passes' widths for this storage", who, (long long)d,
                      (long long)ld);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dw = nullptr, *dz = nullptr, *dlam = nullptr, *dv = nullptr, *partials = nullptr, *red = nullptr;
    RBL_TRY(cols_upload(sc, &dw, W, k, d, ld));
    RBL_TRY(sc.upload(&dz, Z, (size_t)n * k));
    // the slots behind column k - 1 have buffers too, which no launch is told about: they keep their NaN
    RBL_TRY(rows_alloc(sc, &dlam, n, RBL_MULTI_KMAX, LAM, k));
    RBL_TRY(rows_alloc(sc, &dv, n, RBL_MULTI_KMAX, nullptr, 0));
    RBL_TRY(sc.mem.alloc(&partials, (size_t)num_cu * 3 * k));
    RBL_TRY(sc.mem.alloc(&red, (size_t)2 * k));
    const size_t stride = (size_t)n + SWEEP_GUARD;
    const double *pw[RBL_MULTI_KMAX], *pz[RBL_MULTI_KMAX];
    double *pl[RBL_MULTI_KMAX], *pv[RBL_MULTI_KMAX], *pp[RBL_MULTI_KMAX], *pr[RBL_MULTI_KMAX];
    for (int j = 0; j < k; ++j) {
        pw[j] = dw + (size_t)j * ld;
        pz[j] = dz + (size_t)j * n;
        pl[j] = dlam + j * stride;
        pv[j] = dv + j * stride;
        pp[j] = partials + (size_t)j * num_cu * 3;
        pr[j] = red + 2 * j;
    }
    SweepInstance inst{};
    RBL_TRY(launch_sweep_v_multi(storage, Dd, n, ld, k, pw, pz, pl, pv, rho, pp, pr, num_cu, sc.s, &inst));
    RBL_TRY(rows_fetch(sc, who, "lambda", dlam, n, RBL_MULTI_KMAX, LAM_out));
    RBL_TRY(rows_fetch(sc, who, "v", dv, n, RBL_MULTI_KMAX, V));
    double redh[2 * RBL_MULTI_KMAX];
    RBL_HIP(hipMemcpyAsync(redh, red, sizeof(double) * 2 * k, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int j = 0; primal2 && j < k; ++j) primal2[j] = redh[2 * j];
    instance_out(instance, inst);
    return RBL_OK;
}

int rbl_k_sweep_q_multi(int storage, int64_t n, int64_t d, int k, const double* D, const double* Cm, int num_cu, double* Q,
                        int* instance) {
    const char* who = "rbl_k_sweep_q_multi";
    if (k < 1 || k > RBL_MULTI_KMAX) {
        rbl_set_error("%s: %d columns (1..%d)", who, k, RBL_MULTI_KMAX);
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (!sweep_multi_supported(storage, ld)) {
        rbl_set_error("%s: d = %lld (ld = %lld) is outside the multi-column passes' widths for this storage", who, (long long)d,
                      (long long)ld);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, Cm, (size_t)n * k));
    RBL_TRY(sc.mem.alloc(&slab, sweep_multi_slab_doubles(ld, num_cu)));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld * k));
    const double* pc[RBL_MULTI_KMAX];
    double* pq[RBL_MULTI_KMAX];
    for (int j = 0; j < k; ++j) {
        pc[j] = dc + (size_t)j * n;
        pq[j] = dq + (size_t)j * ld;
    }
    SweepInstance inst{};
    RBL_TRY(launch_sweep_q_multi(storage, Dd, n, ld, k, pc, slab, pq, num_cu, sc.s, &inst));
    for (int j = 0; j < k; ++j)
        RBL_HIP(hipMemcpyAsync(Q + (size_t)j * d, dq + (size_t)j * ld, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    instance_out(instance, inst);
    return RBL_OK;
}

// ---- the plain passes (sweep.hip: k_gemv, k_gemvt, its column-statistics variant, k_colreduce) and the Gram kernels on
// prescribed inputs with a caller-chosen grid (rbl_k_pass_*, rbl_k_gram_full): the launchers of a solve, unchanged
namespace {
void pass_out(int* instance, const PassInstance& in) {
    if (!instance) return;
    instance[0] = in.route;
    instance[1] = in.a;
    instance[2] = in.p;
    instance[3] = in.u;
    instance[4] = in.blocks;
    instance[5] = in.tiles;
}
}  // namespace

int rbl_k_pass_v(int storage, int64_t n, int64_t d, const double* D, const double* w, int num_cu, double* v, int* instance) {
    const char* who = "rbl_k_pass_v";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(cols_upload(sc, &dw, w, 1, d, ld));
    RBL_TRY(rows_alloc(sc, &dv, n, 1, nullptr, 0));
    PassInstance inst{};
    RBL_TRY(launch_gemv(storage, Dd, n, ld, dw, dv, num_cu, sc.s, &inst));
    RBL_TRY(rows_fetch(sc, who, "v", dv, n, 1, v));
    pass_out(instance, inst);
    return RBL_OK;
}

int rbl_k_pass_q(int storage, int64_t n, int64_t d, const double* D, const double* c, int num_cu, double* q_ld, int* instance) {
    const char* who = "rbl_k_pass_q";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *dc = nullptr, *slab = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, c, (size_t)n));
    // gemvt_slab_rows(num_cu) rows; where launch_gemvt hands the pass to launch_sweep_q, that launcher's own rule (with the
    // device's CU count the first covers the second, with num_cu = 1 it does not)
    size_t slab_rows = (size_t)gemvt_slab_rows(num_cu);
    if (sweep_v_supported(storage, ld)) slab_rows = std::max(slab_rows, (size_t)sweep_erm_slab_rows(num_cu));
    RBL_TRY(sc.mem.alloc(&slab, slab_rows * ld));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_HIP(hipMemsetAsync(dq, 0xff, sizeof(double) * ld, sc.s));   // (NaN: every entry, the pad included, must be written)
    PassInstance inst{};
    RBL_TRY(launch_gemvt(storage, Dd, n, ld, dc, slab, dq, num_cu, sc.s, nullptr, 0, &inst));
    RBL_HIP(hipMemcpyAsync(q_ld, dq, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    pass_out(instance, inst);
    return RBL_OK;
}

int rbl_k_pass_colstats(int storage, int64_t n, int64_t d, const double* D, int num_cu, double* sum_ld, double* sumsq_ld,
                        int* instance) {
    const char* who = "rbl_k_pass_colstats";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    if (storage == RBL_STORE_F16) {   // refused before anything is uploaded; launch_colstats refuses it as well
        rbl_set_error("%s: colstats: not available for RBL_STORE_F16", who);
        return RBL_ERR_INVALID;
    }
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *slab = nullptr, *ds = nullptr;
    RBL_TRY(sc.mem.alloc(&slab, (size_t)gemvt_slab_rows(num_cu) * ld * 2));   // (sums | sums of squares, as a handle's slab)
    RBL_TRY(sc.mem.alloc(&ds, (size_t)ld * 2));
    RBL_HIP(hipMemsetAsync(ds, 0xff, sizeof(double) * ld * 2, sc.s));
    PassInstance inst{};
    RBL_TRY(launch_colstats(storage, Dd, n, ld, slab, ds, ds + ld, num_cu, sc.s, &inst));
    RBL_HIP(hipMemcpyAsync(sum_ld, ds, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipMemcpyAsync(sumsq_ld, ds + ld, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    pass_out(instance, inst);
    return RBL_OK;
}

int rbl_k_gram_full(int storage, int64_t n, int64_t d, const double* D, int num_cu, double* G_ld, int64_t* plan) {
    const char* who = "rbl_k_gram_full";
    Scratch sc;
    int64_t ld = 0;
    RBL_TRY(sweep_begin(sc, who, storage, n, d, num_cu, &ld));
    void* Dd = nullptr;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *slab = nullptr, *dG = nullptr;
    RBL_TRY(sc.mem.alloc((unsigned char**)&slab, gram_slab_bytes(ld, num_cu, n)));
    RBL_TRY(sc.mem.alloc(&dG, (size_t)ld * ld));
    RBL_HIP(hipMemsetAsync(dG, 0xff, sizeof(double) * ld * ld, sc.s));
    GramPlanOut g{};
    RBL_TRY(launch_gram(storage, Dd, n, ld, d, slab, dG, num_cu, sc.s, &g));
    RBL_HIP(hipMemcpyAsync(G_ld, dG, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (plan) {
        plan[0] = g.ntiles;
        plan[1] = g.npairs;
        plan[2] = g.ksplit;
        plan[3] = g.rows_per_split;
    }
    return RBL_OK;
}

int rbl_k_gram(int storage, int64_t n, int64_t d, const double* D, double* G) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    void* Dd = nullptr;
    int64_t ld = 0;
    RBL_TRY(upload_matrix(sc, storage, n, d, D, &Dd, &ld));
    double *slab = nullptr, *dG = nullptr;
    RBL_TRY(sc.mem.alloc((unsigned char**)&slab, gram_slab_bytes(ld, num_cu, n > 0 ? n : 1)));
    RBL_TRY(sc.mem.alloc(&dG, (size_t)ld * ld));
    RBL_TRY(launch_gram(storage, Dd, n, ld, d, slab, dG, num_cu, sc.s));
    std::vector<double> hG((size_t)ld * ld);
    RBL_HIP(hipMemcpyAsync(hG.data(), dG, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int64_t i = 0; i < d; ++i)
        for (int64_t j = 0; j < d; ++j) G[i * d + j] = hG[(size_t)(i * ld + j)];
    return RBL_OK;
}

int rbl_k_csr_gemv(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, const double* w,
                   double* v) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    if (n <= 0) return RBL_OK;
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, "rbl_k_csr_gemv", n, d, indptr, indices, values, false, num_cu, &st, &ld));
    std::vector<double> wp((size_t)ld, 0.0);
    for (int64_t j = 0; j < d; ++j) wp[(size_t)j] = w[j];
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(sc.upload(&dw, wp.data(), (size_t)ld));
    RBL_TRY(sc.mem.alloc(&dv, (size_t)n));
    RBL_TRY(launch_gemv(RBL_STORE_CSR, &st, n, ld, dw, dv, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(v, dv, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

// q has ld = storage_ld(d) entries here: the padding [d, ld) is part of what the pass writes (+0.0)
int rbl_k_csr_gemvt(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, const double* c,
                    double* q) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, "rbl_k_csr_gemvt", n, d, indptr, indices, values, true, num_cu, &st, &ld));
    double *dc = nullptr, *part = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, c, (size_t)n));
    RBL_TRY(sc.mem.alloc(&part, (size_t)st.nseg));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_HIP(hipMemsetAsync(dq, 0xff, sizeof(double) * ld, sc.s));   // (NaN: every entry must be written by the pass)
    RBL_TRY(launch_gemvt(RBL_STORE_CSR, &st, n, ld, dc, part, dq, num_cu, sc.s, nullptr, (size_t)st.nseg));
    RBL_HIP(hipMemcpyAsync(q, dq, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

// the checks of the two multi-column entries that come before any upload
static int csr_multi_begin(Scratch& sc, const char* who, int k, const void* in, const void* out, int num_cu) {
    if (k < 1 || k > RBL_MULTI_KMAX || !in || !out) {
        rbl_set_error("%s: 1..%d columns (got %d), input and output not NULL", who, RBL_MULTI_KMAX, k);
        return RBL_ERR_INVALID;
    }
    int cus = 0;
    RBL_TRY(scratch_begin(sc, &cus));
    if (num_cu < 1 || num_cu > cus) {
        rbl_set_error("%s: num_cu = %d outside 1..%d (the device's compute units)", who, num_cu, cus);
        return RBL_ERR_INVALID;
    }
    return RBL_OK;
}

int rbl_k_csr_gemv_multi(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int k,
                         const double* W, int num_cu, double* V, int* lanes_out) {
    const char* who = "rbl_k_csr_gemv_multi";
    Scratch sc;
    RBL_TRY(csr_multi_begin(sc, who, k, W, V, num_cu));
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, who, n, d, indptr, indices, values, false, num_cu, &st, &ld));
    double *dw = nullptr, *dv = nullptr;
    RBL_TRY(cols_upload(sc, &dw, W, k, d, ld));
    RBL_TRY(rows_alloc(sc, &dv, n, k, nullptr, 0));
    const double* w[RBL_MULTI_KMAX];
    double* v[RBL_MULTI_KMAX];
    for (int j = 0; j < k; ++j) {
        w[j] = dw + (size_t)j * ld;
        v[j] = dv + (size_t)j * (n + SWEEP_GUARD);
    }
    RBL_TRY(launch_csr_gemv_multi(&st, n, k, w, v, num_cu, sc.s));
    RBL_TRY(rows_fetch(sc, who, "v", dv, n, k, V));
    if (lanes_out) *lanes_out = st.lanes;
    return RBL_OK;
}

int rbl_k_csr_gemvt_multi(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int k,
                          const double* C, int num_cu, double* Q, int64_t* nseg_out) {
    const char* who = "rbl_k_csr_gemvt_multi";
    Scratch sc;
    RBL_TRY(csr_multi_begin(sc, who, k, C, Q, num_cu));
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, who, n, d, indptr, indices, values, true, num_cu, &st, &ld));
    const size_t ks = (size_t)csr_multi_stride(k), part_doubles = (size_t)st.nseg * ks, cp_doubles = (size_t)n * ks;
    double *dc = nullptr, *cp = nullptr, *part = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dc, C, (size_t)n * k));
    RBL_TRY(sc.mem.alloc(&cp, cp_doubles));
    RBL_TRY(sc.mem.alloc(&part, part_doubles));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld * k));
    RBL_HIP(hipMemsetAsync(dq, 0xff, sizeof(double) * ld * k, sc.s));   // (NaN: every entry, the pad included, must be written)
    RBL_HIP(hipMemsetAsync(part, 0xff, sizeof(double) * (part_doubles > 0 ? part_doubles : 1), sc.s));
    const double* c[RBL_MULTI_KMAX];
    double* q[RBL_MULTI_KMAX];
    for (int j = 0; j < k; ++j) {
        c[j] = dc + (size_t)j * n;
        q[j] = dq + (size_t)j * ld;
    }
    RBL_TRY(launch_csr_gemvt_multi(&st, n, ld, k, c, cp, cp_doubles, part, part_doubles, q, num_cu, sc.s));
    RBL_HIP(hipMemcpyAsync(Q, dq, sizeof(double) * ld * k, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (nseg_out) *nseg_out = st.nseg;
    return RBL_OK;
}

int rbl_k_csr_gram(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, double* G) {
    Scratch sc;
    int num_cu = 256;
    RBL_TRY(scratch_begin(sc, &num_cu));
    CsrStore st;
    int64_t ld = 0;
    // the column form where the rule picks the route that walks it (upload_csr checks indptr before it is read again)
    const bool columns = indptr && n >= 1 && d >= 1 && indptr[0] == 0 && indptr[n] >= 0 &&
                         csr_gram_route(n, rbl_storage_ld(RBL_STORE_CSR, d), csr_gram_pair_products(indptr, n, 0)) == CSR_GRAM_ROUTE_SPARSE;
    RBL_TRY(upload_csr(sc, "rbl_k_csr_gram", n, d, indptr, indices, values, columns, num_cu, &st, &ld));
    double *slab = nullptr, *dG = nullptr;
    RBL_TRY(sc.mem.alloc((unsigned char**)&slab, gram_slab_bytes(ld, num_cu, n)));
    RBL_TRY(sc.mem.alloc(&dG, (size_t)ld * ld));
    RBL_TRY(launch_gram(RBL_STORE_CSR, &st, n, ld, d, slab, dG, num_cu, sc.s));
    std::vector<double> hG((size_t)ld * ld);
    RBL_HIP(hipMemcpyAsync(hG.data(), dG, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int64_t i = 0; i < d; ++i)
        for (int64_t j = 0; j < d; ++j) G[i * d + j] = hG[(size_t)(i * ld + j)];
    return RBL_OK;
}

int rbl_k_csr_gram_route(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int route,
                         int num_cu, int tile_cols, double* G_ld, rbl_gram_report* rep) {
    Scratch sc;
    int dev_cu = 256;
    RBL_TRY(scratch_begin(sc, &dev_cu));
    if (num_cu <= 0) num_cu = dev_cu;
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, "rbl_k_csr_gram_route", n, d, indptr, indices, values, true, num_cu, &st, &ld));
    double *slab = nullptr, *dG = nullptr;
    RBL_TRY(sc.mem.alloc((unsigned char**)&slab, gram_slab_bytes(ld, num_cu, n)));
    RBL_TRY(sc.mem.alloc(&dG, (size_t)ld * ld));
    RBL_HIP(hipMemsetAsync(dG, 0xff, sizeof(double) * ld * ld, sc.s));   // (NaN: every entry must be written by the route)
    rbl_gram_report r{};
    RBL_TRY(launch_csr_gram(&st, n, ld, d, slab, dG, num_cu, sc.s, route, tile_cols, &r));
    RBL_HIP(hipMemcpyAsync(G_ld, dG, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (rep) *rep = r;
    return RBL_OK;
}

int rbl_k_wstep(int wstep, int64_t d, const double* G, const double* q, double rho, double reg, double smooth_t,
                const double* w0, double tol, double* w_out, int* iters) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    const int64_t ld = round_up(d, 4);
    std::vector<double> hG((size_t)ld * ld, 0.0), hq((size_t)ld, 0.0), hw((size_t)ld, 0.0);
    for (int64_t i = 0; i < d; ++i) {
        for (int64_t j = 0; j < d; ++j) hG[(size_t)(i * ld + j)] = G[i * d + j];
        hq[(size_t)i] = q[i];
        hw[(size_t)i] = w0 ? w0[i] : 0.0;
    }
    double *dG = nullptr, *dq = nullptr, *dw = nullptr;
    RBL_TRY(sc.upload(&dG, hG.data(), hG.size()));
    RBL_TRY(sc.upload(&dq, hq.data(), hq.size()));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    double lam = 0.0;
    RBL_TRY(launch_power_iteration(dG, ld, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    int it = 0;
    RBL_TRY(run_wstep(wstep, dG, ld, dq, rho, reg, smooth_t, L, tol > 0.0 ? tol : 1e-13, 100000, dw, ww, &it, sc.s));
    RBL_HIP(hipMemcpyAsync(w_out, dw, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (iters) *iters = it;
    return RBL_OK;
}

int rbl_k_wstep_pen(int64_t d, const double* G, const double* q, double rho, const double* l1, const double* l2,
                    const double* w0, double tol, double* w_out, int* iters, int* form) {
    if (d <= 0 || !G || !q || !w_out || (!l1 && !l2) || !(rho > 0.0)) {
        rbl_set_error("k_wstep_pen: bad argument (d > 0, G, q, w_out, rho > 0 and l1 or l2 are needed)");
        return RBL_ERR_INVALID;
    }
    bool any_l1 = false;
    double l2max = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double* v = k ? l2 : l1;
        for (int64_t j = 0; v && j < d; ++j) {
            if (!(v[j] >= 0.0) || !std::isfinite(v[j])) {
                rbl_set_error("k_wstep_pen: %s[%lld] = %g - penalties must be finite and >= 0", k ? "l2" : "l1", (long long)j,
                              v[j]);
                return RBL_ERR_INVALID;
            }
            if (!k && v[j] > 0.0) any_l1 = true;
            if (k && v[j] > l2max) l2max = v[j];
        }
    }
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    const int64_t ld = round_up(d, 4);
    std::vector<double> hG((size_t)ld * ld, 0.0), hq((size_t)ld, 0.0), hw((size_t)ld, 0.0), hp((size_t)(2 * ld), 0.0);
    for (int64_t i = 0; i < d; ++i) {
        for (int64_t j = 0; j < d; ++j) hG[(size_t)(i * ld + j)] = G[i * d + j];
        hq[(size_t)i] = q[i];
        hw[(size_t)i] = w0 ? w0[i] : 0.0;
        hp[(size_t)i] = l1 ? l1[i] : 0.0;
        hp[(size_t)(ld + i)] = l2 ? l2[i] : 0.0;
    }
    double *dG = nullptr, *dq = nullptr, *dw = nullptr, *dp = nullptr;
    RBL_TRY(sc.upload(&dG, hG.data(), hG.size()));
    RBL_TRY(sc.upload(&dq, hq.data(), hq.size()));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    RBL_TRY(sc.upload(&dp, hp.data(), hp.size()));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    ww.pen_l1 = dp;
    ww.pen_l2 = dp + ld;
    ww.pen_l2max = l2max;
    double lam = 0.0;
    RBL_TRY(launch_power_iteration(dG, ld, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    int it = 0;
    RBL_TRY(run_wstep(any_l1 ? RBL_WSTEP_L1 : RBL_WSTEP_L2, dG, ld, dq, rho, 0.0, 1.0, L, tol > 0.0 ? tol : 1e-13, 100000, dw,
                      ww, &it, sc.s));
    RBL_HIP(hipMemcpyAsync(w_out, dw, sizeof(double) * d, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (iters) *iters = it;
    if (form) *form = ww.form;
    return RBL_OK;
}

// The operator w-step (wstep_op.hip) as a handle created with RBL_CREATE_NO_GRAM runs it: the entries are uploaded and both
// forms built, L comes from the power iteration through the operator, then one run_wstep_op
int rbl_k_wstep_op(int wstep, int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values,
                   const double* q, double rho, double reg, const double* l1, const double* l2, double tol, int max_inner,
                   int num_cu, double* w_inout, int* iters, int* status) {
    const char* who = "rbl_k_wstep_op";
    if (wstep == RBL_WSTEP_SMOOTH_L1) {
        rbl_set_error("%s: no smoothed-l1 w-step on the operator route (RBL_WSTEP_SMOOTH_L1 preconditions with diag(G), and there "
                      "is no Gram matrix)", who);
        return RBL_ERR_INVALID;
    }
    if (wstep != RBL_WSTEP_L1 && wstep != RBL_WSTEP_L2) {
        rbl_set_error("%s: wstep must be 1 (lasso / elastic net) or 2 (ridge), got %d", who, wstep);
        return RBL_ERR_INVALID;
    }
    const bool pen = l1 || l2;
    if (d < 1 || n < 1 || !indptr || !q || !w_inout || !(rho > 0.0) || !std::isfinite(rho) || max_inner < 1 || !std::isfinite(tol) ||
        (!pen && (!(reg > 0.0) || !std::isfinite(reg)))) {
        rbl_set_error("%s: bad argument (n >= 1, d >= 1, indptr, q, w_inout, finite rho > 0, max_inner >= 1, and a finite reg > 0 "
                      "or l1 / l2 are needed; n = %lld, d = %lld)", who, (long long)n, (long long)d);
        return RBL_ERR_INVALID;
    }
    double l2max = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double* v = k ? l2 : l1;
        for (int64_t j = 0; v && j < d; ++j) {
            if (!(v[j] >= 0.0) || !std::isfinite(v[j])) {
                rbl_set_error("%s: %s[%lld] = %g - penalties must be finite and >= 0", who, k ? "l2" : "l1", (long long)j, v[j]);
                return RBL_ERR_INVALID;
            }
            if (k && v[j] > l2max) l2max = v[j];
        }
    }
    Scratch sc;
    int cus = 0;
    RBL_TRY(scratch_begin(sc, &cus));
    if (num_cu == 0) num_cu = cus;
    if (num_cu < 1 || num_cu > cus) {
        rbl_set_error("%s: num_cu = %d outside 1..%d (the device's compute units; 0 = all)", who, num_cu, cus);
        return RBL_ERR_INVALID;
    }
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, who, n, d, indptr, indices, values, true, num_cu, &st, &ld));
    std::vector<double> hq((size_t)ld, 0.0), hw((size_t)ld, 0.0), hp((size_t)(2 * ld), 0.0);
    for (int64_t i = 0; i < d; ++i) {
        hq[(size_t)i] = q[i];
        hw[(size_t)i] = w_inout[i];
        hp[(size_t)i] = l1 ? l1[i] : 0.0;
        hp[(size_t)(ld + i)] = l2 ? l2[i] : 0.0;
    }
    double *dq = nullptr, *dw = nullptr, *dp = nullptr;
    RBL_TRY(sc.upload(&dq, hq.data(), hq.size()));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    if (pen) {
        RBL_TRY(sc.upload(&dp, hp.data(), hp.size()));
        ww.pen_l1 = dp;
        ww.pen_l2 = dp + ld;
        ww.pen_l2max = l2max;
    }
    OpData op{&st, n, nullptr, nullptr, (size_t)(st.nseg > 0 ? st.nseg : 1), nullptr, num_cu};
    RBL_TRY(sc.mem.alloc(&op.t, (size_t)n));
    RBL_TRY(sc.mem.alloc(&op.slab, op.slab_doubles));
    RBL_TRY(sc.mem.alloc(&op.part, op_part_doubles(ld)));
    double lam = 0.0;
    RBL_TRY(launch_op_power_iteration(op, ld, d, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    int it = 0;
    RBL_TRY(run_wstep_op(wstep, op, ld, dq, rho, reg, L, tol > 0.0 ? tol : 1e-13, max_inner, dw, ww, &it, sc.s));
    RBL_HIP(hipMemcpyAsync(w_inout, dw, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    if (iters) *iters = it;
    if (status) *status = reinterpret_cast<const volatile int*>(ww.pin)[wstep == RBL_WSTEP_L2 ? 4 : 6] == 1 ? 1 : 0;
    return RBL_OK;
}

// ---- the working-set lasso (wstep_ws.hip) piece by piece and as a handle runs it
int rbl_k_wset_gram(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* cols,
                    int ncols, const int32_t* split, int nsplit, int num_cu, double* Gs_out) {
    const char* who = "rbl_k_wset_gram";
    if (ncols < 0 || ncols > WS_CAP || (ncols > 0 && !cols) || !Gs_out || (split && nsplit < 1)) {
        rbl_set_error("%s: bad argument (0 <= ncols <= %d, cols, Gs_out; split needs nsplit >= 1)", who, WS_CAP);
        return RBL_ERR_INVALID;
    }
    std::vector<char> seen((size_t)(d > 0 ? d : 1), 0);
    for (int i = 0; i < ncols; ++i) {
        if (cols[i] < 0 || cols[i] >= d || seen[(size_t)cols[i]]) {
            rbl_set_error("%s: cols[%d] = %d is outside [0, %lld) or appears twice", who, i, cols[i], (long long)d);
            return RBL_ERR_INVALID;
        }
        seen[(size_t)cols[i]] = 1;
    }
    int64_t total = 0;
    for (int k = 0; split && k < nsplit; ++k) {
        if (split[k] < 0) total = -1;
        if (total >= 0) total += split[k];
    }
    if (split && total != ncols) {
        rbl_set_error("%s: the calls of split add up to %lld columns, ncols = %d", who, (long long)total, ncols);
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    int cus = 0;
    RBL_TRY(scratch_begin(sc, &cus));
    if (num_cu == 0) num_cu = cus;
    if (num_cu < 1 || num_cu > cus) {
        rbl_set_error("%s: num_cu = %d outside 1..%d (the device's compute units; 0 = all)", who, num_cu, cus);
        return RBL_ERR_INVALID;
    }
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, who, n, d, indptr, indices, values, true, num_cu, &st, &ld));
    WsetState W;
    RBL_TRY(alloc_wset(sc.mem, W, ld, sc.s));
    std::vector<int> c(cols, cols + ncols);
    if (!split) {
        RBL_TRY(wset_gram(&st, W, ld, c.data(), ncols, num_cu, sc.s));
    } else {
        int at = 0;
        for (int k = 0; k < nsplit; ++k) {
            RBL_TRY(wset_gram(&st, W, ld, c.data() + at, split[k], num_cu, sc.s));
            at += split[k];
        }
    }
    RBL_HIP(hipMemcpyAsync(Gs_out, W.Gs, sizeof(double) * (size_t)WS_CAP * WS_CAP, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

int rbl_k_wset_scan(int64_t ld, int64_t d, const double* g, const double* kappa, const double* q, const int32_t* member, double tol,
                    int take, int32_t* cols_out, int* count) {
    const char* who = "rbl_k_wset_scan";
    if (ld < 2 || (ld & 1) || d < 1 || d > ld || ld > 0x7fffffffLL || !g || !kappa || !member || !cols_out || !count || take < 0 ||
        take > WS_SELECT || !std::isfinite(tol)) {
        rbl_set_error("%s: bad argument (ld even, 1 <= d <= ld, g, kappa, member, cols_out, count, 0 <= take <= %d are needed)", who,
                      WS_SELECT);
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    WsetState W;
    RBL_TRY(alloc_wset(sc.mem, W, ld, sc.s, true));
    double *dg = nullptr, *dk = nullptr, *dq = nullptr;
    RBL_TRY(sc.upload(&dg, g, (size_t)ld));
    RBL_TRY(sc.upload(&dk, kappa, (size_t)ld));
    if (q) RBL_TRY(sc.upload(&dq, q, (size_t)ld));
    std::vector<int> pos((size_t)ld);
    for (int64_t j = 0; j < ld; ++j) pos[(size_t)j] = member[j] ? 0 : -1;
    int cnt = 0, sel[WS_SELECT];
    RBL_TRY(wset_scan(W, ld, d, dg, dq, dk, pos.data(), tol, take, &cnt, sel, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    for (int i = 0; i < cnt; ++i) cols_out[i] = sel[i];
    *count = cnt;
    return RBL_OK;
}

int rbl_k_wstep_ws(int64_t n, int64_t d, const int64_t* indptr, const int32_t* indices, const double* values, int K,
                   const double* Q, double rho, double reg, const double* l1, const double* l2, double tol, int max_inner,
                   int num_cu, int ws_cap, const double* w0, double* W_out, rbl_wset_report* reports) {
    const char* who = "rbl_k_wstep_ws";
    const bool pen = l1 || l2;
    if (d < 1 || n < 1 || K < 1 || !indptr || !Q || !W_out || !reports || !(rho > 0.0) || !std::isfinite(rho) || max_inner < 1 ||
        !std::isfinite(tol) || ws_cap < 0 || ws_cap > WS_CAP || (!pen && (!(reg > 0.0) || !std::isfinite(reg)))) {
        rbl_set_error("%s: bad argument (n, d, K >= 1, indptr, Q, W_out, reports, finite rho > 0, max_inner >= 1, 0 <= ws_cap <= %d, "
                      "and a finite reg > 0 or l1 / l2 are needed; n = %lld, d = %lld)", who, WS_CAP, (long long)n, (long long)d);
        return RBL_ERR_INVALID;
    }
    double l2max = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double* v = k ? l2 : l1;
        for (int64_t j = 0; v && j < d; ++j) {
            if (!(v[j] >= 0.0) || !std::isfinite(v[j])) {
                rbl_set_error("%s: %s[%lld] = %g - penalties must be finite and >= 0", who, k ? "l2" : "l1", (long long)j, v[j]);
                return RBL_ERR_INVALID;
            }
            if (k && v[j] > l2max) l2max = v[j];
        }
    }
    Scratch sc;
    int cus = 0;
    RBL_TRY(scratch_begin(sc, &cus));
    if (num_cu == 0) num_cu = cus;
    if (num_cu < 1 || num_cu > cus) {
        rbl_set_error("%s: num_cu = %d outside 1..%d (the device's compute units; 0 = all)", who, num_cu, cus);
        return RBL_ERR_INVALID;
    }
    CsrStore st;
    int64_t ld = 0;
    RBL_TRY(upload_csr(sc, who, n, d, indptr, indices, values, true, num_cu, &st, &ld));
    std::vector<double> hQ((size_t)(K * ld), 0.0), hw((size_t)ld, 0.0), hp((size_t)(2 * ld), 0.0), hl1((size_t)d, 0.0);
    for (int k = 0; k < K; ++k)
        for (int64_t i = 0; i < d; ++i) hQ[(size_t)(k * ld + i)] = Q[(size_t)k * d + i];
    for (int64_t i = 0; i < d; ++i) {
        hw[(size_t)i] = w0 ? w0[i] : 0.0;
        hp[(size_t)i] = hl1[(size_t)i] = l1 ? l1[i] : 0.0;
        hp[(size_t)(ld + i)] = l2 ? l2[i] : 0.0;
    }
    double *dQ = nullptr, *dw = nullptr, *dp = nullptr;
    RBL_TRY(sc.upload(&dQ, hQ.data(), hQ.size()));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    if (pen) {
        RBL_TRY(sc.upload(&dp, hp.data(), hp.size()));
        ww.pen_l1 = dp;
        ww.pen_l2 = dp + ld;
        ww.pen_l2max = l2max;
    }
    OpData op{&st, n, nullptr, nullptr, (size_t)(st.nseg > 0 ? st.nseg : 1), nullptr, num_cu};
    RBL_TRY(sc.mem.alloc(&op.t, (size_t)n));
    RBL_TRY(sc.mem.alloc(&op.slab, op.slab_doubles));
    RBL_TRY(sc.mem.alloc(&op.part, op_part_doubles(ld)));
    WsetState W;
    RBL_TRY(alloc_wset(sc.mem, W, ld, sc.s));
    double lam = 0.0;
    RBL_TRY(launch_op_power_iteration(op, ld, d, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    for (int k = 0; k < K; ++k) {
        int it = 0;
        RBL_TRY(run_wstep_ws(op, ld, d, dQ + (size_t)k * ld, rho, reg, L, tol > 0.0 ? tol : 1e-13, max_inner, dw, ww, W,
                             ws_cap > 0 ? ws_cap : WS_CAP, pen ? hl1.data() : nullptr, &it, sc.s));
        RBL_HIP(hipMemcpyAsync(W_out + (size_t)k * ld, dw, sizeof(double) * ld, hipMemcpyDeviceToHost, sc.s));
        RBL_HIP(hipStreamSynchronize(sc.s));
        reports[k] = W.rep;
    }
    return RBL_OK;
}

int rbl_k_wstep_seq(int wstep, int64_t d, const double* G, int K, const double* Q, double rho, double reg, double smooth_t,
                    const double* l1, const double* l2, const double* w0, double tol, int max_inner, int route,
                    int launch_seq0, int flags, double* W, double* Gw, double* Wprev, rbl_wstep_report* reports) {
    const char* who = "rbl_k_wstep_seq";
    const bool pen = l1 || l2;
    if (wstep != RBL_WSTEP_L1 && wstep != RBL_WSTEP_L2 && wstep != RBL_WSTEP_SMOOTH_L1) {
        rbl_set_error("%s: wstep must be 1 (lasso), 2 (ridge) or 3 (smoothed l1), got %d", who, wstep);
        return RBL_ERR_INVALID;
    }
    if (d < 1 || d > 16384 || K < 1 || !G || !Q || !W) {
        rbl_set_error("%s: 1 <= d <= 16384, K >= 1, G, Q and W are needed (d = %lld, K = %d)", who, (long long)d, K);
        return RBL_ERR_INVALID;
    }
    if (!(rho > 0.0) || !std::isfinite(rho) || !(reg >= 0.0) || !std::isfinite(reg) || !(tol > 0.0) || !(tol < 1.0) ||
        max_inner < 1 || (wstep == RBL_WSTEP_SMOOTH_L1 && (!(smooth_t > 0.0) || !std::isfinite(smooth_t)))) {
        rbl_set_error("%s: rho > 0, reg >= 0, 0 < tol < 1, max_inner >= 1 and smooth_t > 0 are needed (rho = %g, reg = %g, "
                      "tol = %g, max_inner = %d, smooth_t = %g)", who, rho, reg, tol, max_inner, smooth_t);
        return RBL_ERR_INVALID;
    }
    if (route < 0 || route > 2 || launch_seq0 < 0 || launch_seq0 > 0xfffff ||
        (flags & ~(RBL_KW_WANT_GW | RBL_KW_W_PREV | RBL_KW_RHO_DEV | RBL_KW_TWO_CALL)) != 0) {
        rbl_set_error("%s: route is 0, 1 or 2, 0 <= launch_seq0 <= 0xfffff, flags are RBL_KW_* (route = %d, launch_seq0 = %d, "
                      "flags = %d)", who, route, launch_seq0, flags);
        return RBL_ERR_INVALID;
    }
    if (route == 2 && wstep != RBL_WSTEP_L2) {
        rbl_set_error("%s: route 2 (the eigendecomposition ridge) goes with wstep 2, got wstep %d", who, wstep);
        return RBL_ERR_INVALID;
    }
    if (pen && wstep == RBL_WSTEP_SMOOTH_L1) {
        rbl_set_error("%s: per-coordinate penalties go with wstep 1 or 2", who);
        return RBL_ERR_INVALID;
    }
    if (wstep != RBL_WSTEP_L1 && (flags & (RBL_KW_W_PREV | RBL_KW_RHO_DEV | RBL_KW_TWO_CALL)) != 0) {
        rbl_set_error("%s: RBL_KW_W_PREV, RBL_KW_RHO_DEV and RBL_KW_TWO_CALL are call forms of the lasso (wstep 1)", who);
        return RBL_ERR_INVALID;
    }
    if (((flags & RBL_KW_WANT_GW) && !Gw) || ((flags & RBL_KW_W_PREV) && !Wprev)) {
        rbl_set_error("%s: RBL_KW_WANT_GW needs Gw, RBL_KW_W_PREV needs Wprev", who);
        return RBL_ERR_INVALID;
    }
    double l2max = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double* v = k ? l2 : l1;
        for (int64_t j = 0; v && j < d; ++j) {
            if (!(v[j] >= 0.0) || !std::isfinite(v[j])) {
                rbl_set_error("%s: %s[%lld] = %g - penalties must be finite and >= 0", who, k ? "l2" : "l1", (long long)j, v[j]);
                return RBL_ERR_INVALID;
            }
            if (k && v[j] > l2max) l2max = v[j];
        }
    }
    const bool want_Gw = (flags & RBL_KW_WANT_GW) != 0, want_prev = (flags & RBL_KW_W_PREV) != 0;
    const bool rho_on_dev = (flags & RBL_KW_RHO_DEV) != 0, two_call = rho_on_dev || (flags & RBL_KW_TWO_CALL) != 0;

    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    const int64_t ld = round_up(d, 4);
    std::vector<double> hG((size_t)ld * ld, 0.0), hq((size_t)ld, 0.0), hw((size_t)ld, 0.0), hp((size_t)(2 * ld), 0.0);
    for (int64_t i = 0; i < d; ++i) {
        for (int64_t j = 0; j < d; ++j) hG[(size_t)(i * ld + j)] = G[i * d + j];
        hw[(size_t)i] = w0 ? w0[i] : 0.0;
        hp[(size_t)i] = l1 ? l1[i] : 0.0;
        hp[(size_t)(ld + i)] = l2 ? l2[i] : 0.0;
    }
    double *dG = nullptr, *dq = nullptr, *dw = nullptr, *dp = nullptr, *dprev = nullptr, *drho = nullptr;
    RBL_TRY(sc.upload(&dG, hG.data(), hG.size()));
    RBL_TRY(sc.mem.alloc(&dq, (size_t)ld));
    RBL_TRY(sc.upload(&dw, hw.data(), hw.size()));
    RBL_TRY(sc.upload(&dp, hp.data(), hp.size()));
    RBL_TRY(sc.mem.alloc(&dprev, (size_t)ld));
    RBL_TRY(sc.upload(&drho, &rho, 1));
    WstepWorkspace ww{};
    RBL_TRY(alloc_wstep(sc.mem, ww, ld, sc.s));
    if (pen) {
        ww.pen_l1 = dp;
        ww.pen_l2 = dp + ld;
        ww.pen_l2max = l2max;
    }
    if (route == 1) ww.bar = nullptr, ww.xch = nullptr;   // run_wstep takes the persistent route only with both
    ww.launch_seq = launch_seq0;
    WstepInstance inst{};
    ww.inst = &inst;
    double lam = 0.0;
    RBL_TRY(launch_power_iteration(dG, ld, ww.yk, ww.Gy, ww.scal, 100, &lam, sc.s));
    double L = 1.02 * lam;
    if (!(L > 0.0)) L = 1.0;
    if (route == 2 && ld <= 2048) {   // the decomposition as rbl_gram_finish runs it
        const size_t nn = (size_t)ld * (size_t)ld;
        RBL_TRY(sc.mem.alloc(&ww.eig_Vt, nn));
        RBL_TRY(sc.mem.alloc(&ww.eig_V, nn));
        RBL_TRY(sc.mem.alloc(&ww.eig_lambda, (size_t)ld));
        int rc = RBL_OK, sweeps = 0;
        {
            DevArena tmp;   // Jacobi scratch, freed after the stream wait
            double* Bt = nullptr;
            unsigned long long* off = nullptr;
            RBL_TRY(tmp.alloc(&Bt, nn));
            RBL_TRY(tmp.alloc(&off, 1));
            rc = launch_eig_jacobi(dG, ld, d, Bt, ww.eig_Vt, ww.eig_V, ww.eig_lambda, off, sc.s, &sweeps);
            (void)hipStreamSynchronize(sc.s);
        }
        RBL_TRY(rc);
        ww.eig_ok = sweeps > 0;
    }
    int dev = 0;
    RBL_HIP(hipGetDevice(&dev));
    const size_t row = sizeof(double) * (size_t)d;
    for (int k = 0; k < K; ++k) {
        for (int64_t i = 0; i < d; ++i) hq[(size_t)i] = Q[(size_t)k * d + i];
        RBL_HIP(hipMemcpyAsync(dq, hq.data(), sizeof(double) * ld, hipMemcpyHostToDevice, sc.s));
        RBL_HIP(hipMemsetAsync(dprev, 0xff, sizeof(double) * ld, sc.s));   // NaN: what the kernel does not save stays so
        RBL_HIP(hipStreamSynchronize(sc.s));                              // (hq is reused)
        inst = WstepInstance{};
        int it = 0;
        bool fs_pending = false, fell_back = false;
        RBL_TRY(run_wstep(wstep, dG, ld, dq, rho_on_dev ? 1.0 : rho, reg, smooth_t, L, tol, max_inner, dw, ww, &it, sc.s,
                          two_call ? &fs_pending : nullptr, rho_on_dev ? drho : nullptr, want_prev ? dprev : nullptr, want_Gw));
        if (fs_pending)
            RBL_TRY(finish_wstep_l1(dG, ld, dq, rho, pen ? 0.0 : reg, L, tol, max_inner, dw, ww, &it, sc.s, &fell_back));
        RBL_HIP(hipStreamSynchronize(sc.s));
        const volatile int* pin = ww.pin;
        const bool lasso = wstep == RBL_WSTEP_L1;
        if (lasso && !two_call) fell_back = ww.form != 2;
        const bool gw_ok = want_Gw && (lasso ? (pin[0] == 0 && ww.form == 2) : ww.gw_valid);
        RBL_HIP(hipMemcpy(W + (size_t)k * d, dw, row, hipMemcpyDeviceToHost));
        if (Gw) {
            if (gw_ok) RBL_HIP(hipMemcpy(Gw + (size_t)k * d, ww.Gy, row, hipMemcpyDeviceToHost));
            else memset(Gw + (size_t)k * d, 0xff, row);
        }
        if (Wprev) RBL_HIP(hipMemcpy(Wprev + (size_t)k * d, dprev, row, hipMemcpyDeviceToHost));
        if (reports) {
            rbl_wstep_report& r = reports[k];
            memset(&r, 0, sizeof(r));
            r.form = ww.form;
            r.iters = it;
            r.phase_a = -1;
            if (lasso) {
                for (int i = 0; i < 4; ++i) r.fs[i] = pin[i];
                r.status = pin[0];
            } else {
                r.status = wstep == RBL_WSTEP_L2 ? pin[4] : pin[8];
            }
            if (inst.nblocks > 0) {   // a persistent launch ran (form 0 with one: its iteration cap handed over to FISTA)
                r.glds = inst.glds;
                r.per = inst.per;
                r.nblocks = inst.nblocks;
                r.lds_bytes = inst.lds_bytes;
                if (wstep == RBL_WSTEP_SMOOTH_L1) r.phase_a = pin[10];
            }
            r.fell_back = fell_back ? 1 : 0;
            r.gw_valid = gw_ok ? 1 : 0;
            r.last_iters = ww.last_iters;
            r.last_fista = ww.last_fista;
            r.ncg_skip = ww.ncg_skip;
            r.ncg_backoff = ww.ncg_backoff;
            r.launch_seq = ww.launch_seq;
            r.live_handles = rbl_live_handles(dev);
        }
    }
    return RBL_OK;
}

int rbl_k_eig(int64_t d, const double* G, double* Vt_ld, double* V_ld, double* lambda_ld, int64_t* ld_out, int* sweeps_out) {
    const char* who = "rbl_k_eig";
    if (d < 1 || d > 2048 || !G || !Vt_ld || !V_ld || !lambda_ld || !ld_out || !sweeps_out) {
        rbl_set_error("%s: 1 <= d <= 2048 (the width up to which the solver decomposes G), G, Vt_ld, V_ld, lambda_ld, ld and "
                      "sweeps are needed (d = %lld)", who, (long long)d);
        return RBL_ERR_INVALID;
    }
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    const int64_t ld = round_up(d, 4);
    const size_t nn = (size_t)ld * (size_t)ld;
    std::vector<double> hG(nn, 0.0);
    for (int64_t i = 0; i < d; ++i)
        for (int64_t j = 0; j < d; ++j) hG[(size_t)(i * ld + j)] = G[i * d + j];
    double *dG = nullptr, *Bt = nullptr, *Vt = nullptr, *V = nullptr, *lambda = nullptr;
    unsigned long long* off = nullptr;
    RBL_TRY(sc.upload(&dG, hG.data(), hG.size()));
    RBL_TRY(sc.mem.alloc(&Bt, nn));
    RBL_TRY(sc.mem.alloc(&Vt, nn));
    RBL_TRY(sc.mem.alloc(&V, nn));
    RBL_TRY(sc.mem.alloc(&lambda, (size_t)ld));
    RBL_TRY(sc.mem.alloc(&off, 1));
    RBL_HIP(hipMemsetAsync(Vt, 0xff, sizeof(double) * nn, sc.s));   // (NaN: what the decomposition does not write stays so)
    RBL_HIP(hipMemsetAsync(V, 0xff, sizeof(double) * nn, sc.s));
    RBL_HIP(hipMemsetAsync(lambda, 0xff, sizeof(double) * ld, sc.s));
    int sweeps = 0;
    const int rc = launch_eig_jacobi(dG, ld, d, Bt, Vt, V, lambda, off, sc.s, &sweeps);
    (void)hipStreamSynchronize(sc.s);
    RBL_TRY(rc);
    RBL_HIP(hipMemcpy(Vt_ld, Vt, sizeof(double) * nn, hipMemcpyDeviceToHost));
    RBL_HIP(hipMemcpy(V_ld, V, sizeof(double) * nn, hipMemcpyDeviceToHost));
    RBL_HIP(hipMemcpy(lambda_ld, lambda, sizeof(double) * ld, hipMemcpyDeviceToHost));
    *ld_out = ld;
    *sweeps_out = sweeps;
    return RBL_OK;
}

int rbl_k_weights(int weight_function, int64_t n, const double* args, int n_args, double* alphas, double* betas) {
    Scratch sc;
    RBL_TRY(scratch_begin(sc, nullptr));
    if (weight_function < RBL_W_ERM || weight_function > RBL_W_EHRM) {
        rbl_set_error("Unrecognized framework! Options: ['erm','extremile','superquantile','esrm','aorr','aorr_dc','ehrm']");
        return RBL_ERR_INVALID;
    }
    if (weight_function != RBL_W_ERM && weight_function != RBL_W_EHRM) {
        const int need = (weight_function == RBL_W_AORR || weight_function == RBL_W_AORR_DC) ? 2 : 1;
        if (!args || n_args < need) {
            rbl_set_error("args for framework is None!");
            return RBL_ERR_INVALID;
        }
    }
    double a2[2] = {args && n_args > 0 ? args[0] : 0.0, args && n_args > 1 ? args[1] : 0.0};
    double *da = nullptr, *db = nullptr;
    RBL_TRY(sc.mem.alloc(&da, (size_t)n));
    RBL_TRY(sc.mem.alloc(&db, (size_t)n));
    RBL_TRY(launch_weights(weight_function, n, a2, da, db, sc.s));
    if (alphas) RBL_HIP(hipMemcpyAsync(alphas, da, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    if (betas) RBL_HIP(hipMemcpyAsync(betas, db, sizeof(double) * n, hipMemcpyDeviceToHost, sc.s));
    RBL_HIP(hipStreamSynchronize(sc.s));
    return RBL_OK;
}

}  // extern "C"
