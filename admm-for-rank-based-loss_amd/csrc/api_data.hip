// api_data.hip - the data path of a solver handle: rbl_set_data / rbl_set_data_from (X in the caller's type, from host
// or device memory, optional column scaling), the synthetic generator's host side, penalties, labels, the one-vs-rest
// decision, the Gram matrix and rbl_get_D.
#include "api_internal.h"
#include "csr_plan.h"
#include "csr_gram_plan.h"

// ---- rbl_set_data_from: X in the caller's type, from host or device memory ------------------------------------------
static inline size_t src_esz(int dtype) { return dtype == RBL_DTYPE_F16 ? 2 : dtype == RBL_DTYPE_F32 ? 4 : 8; }
static inline double src_host_widen(const void* p, int dtype) {
    if (dtype == RBL_DTYPE_F16) return (double)(float)__builtin_bit_cast(_Float16, *(const unsigned short*)p);
    if (dtype == RBL_DTYPE_F32) return (double)*(const float*)p;
    return *(const double*)p;
}
// first and last byte of the claimed range must be device memory of the handle's device (a host pointer must fail here,
// with a message, not fault in a kernel)
static int src_check_device_range(const void* X, size_t bytes, int device, const char* who = "set_data_from",
                                  const char* what = "X") {
    const char* ends[2] = {(const char*)X, (const char*)X + (bytes ? bytes - 1 : 0)};
    for (const char* p : ends) {
        hipPointerAttribute_t a;
        const hipError_t e = hipPointerGetAttributes(&a, p);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || a.type != hipMemoryTypeDevice) {
            rbl_set_error("%s: %s was passed as RBL_MEM_DEVICE but %p is not device memory (a host array goes "
                          "with RBL_MEM_HOST)", who, what, (const void*)p);
            return RBL_ERR_INVALID;
        }
        if (a.device != device) {
            rbl_set_error("%s: %s lives on device %d, the handle on device %d", who, what, a.device, device);
            return RBL_ERR_INVALID;
        }
    }
    return RBL_OK;
}
// A CSR source as rbl_set_data_csr got it, with the host copy of indptr that plans the chunks
struct CsrView {
    const void *indptr = nullptr, *indices = nullptr, *values = nullptr;
    int64_t nnz = 0;
    int index_type = RBL_INDEX_I32, dtype = RBL_DTYPE_F64, mem = RBL_MEM_HOST;
    size_t isz = 4, esz = 8;
    const int64_t* ip = nullptr;   // n + 1 entries, checked (csr_check_indptr)
    int64_t ds = 0, ldc = 0;       // source columns; row stride of the dense staging chunk (elements, 16-byte rows)
    u64* err = nullptr;            // device: {entries refused by the expand kernel, smallest row that has one}
};
// The upload pipeline of a host source of any element type: the caller's rows are pinned in place and go over
// PCIe untouched, chunk by chunk, into two staging buffers (the copy of chunk k + 1 runs on a second stream while the
// kernels of chunk k read staging buffer k & 1).  A device source is one "chunk": the caller's own memory.  A CSR source
// (pass_csr) of either memory kind is expanded chunk by chunk into ONE dense staging buffer; of a host source the slices of
// its three arrays take the place of the rows in the double-buffered copies.
struct SrcPipe {
    DevArena tmp;
    unsigned char* Xd[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr, copy_stream = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, formed[2] = {nullptr, nullptr};
    void* registered[3] = {nullptr, nullptr, nullptr};   // (a CSR source: three arrays)
    // a CSR source: one dense staging chunk, and for a host source two sets of slices of the three arrays
    unsigned char *stage = nullptr, *ipd[2] = {nullptr, nullptr}, *idx[2] = {nullptr, nullptr}, *val[2] = {nullptr, nullptr};
    ~SrcPipe() {   // (the arena's buffers are freed after this body: nothing may still be running on them)
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        (void)hipStreamSynchronize(stream);
        for (int k = 0; k < 2; ++k) {
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            if (formed[k]) (void)hipEventDestroy(formed[k]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (void* r : registered)
            if (r) (void)hipHostUnregister(r);
        (void)hipGetLastError();
    }
    void pin(const void* X, size_t xbytes, int slot) {
        if (!X || !xbytes) return;
        if (hipHostRegister(const_cast<void*>(X), xbytes, hipHostRegisterDefault) == hipSuccess) registered[slot] = const_cast<void*>(X);
        else (void)hipGetLastError();   // pageable copies instead: slower, same result
    }
    int open_host(const void* X, size_t xbytes, size_t chunk_bytes) {
        pin(X, xbytes, 0);
        RBL_TRY(tmp.alloc(&Xd[0], chunk_bytes));
        RBL_TRY(tmp.alloc(&Xd[1], chunk_bytes));
        return open_copy_stream();
    }
    int open_copy_stream() {
        RBL_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            RBL_HIP(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
            RBL_HIP(hipEventCreateWithFlags(&formed[k], hipEventDisableTiming));
        }
        return RBL_OK;
    }
    // one pass over the source: fn(rows on the device, first row, row count) enqueues its kernels on `stream`; returns
    // with both streams idle
    int pass(const void* X, int mem, size_t esz, int64_t ldx, int64_t ds, int64_t n, int64_t chunk,
             const std::function<int(const void*, int64_t, int64_t)>& fn, double* ms = nullptr) {
        return timed(ms, [&]() {
            if (mem == RBL_MEM_DEVICE) return fn(X, (int64_t)0, n);
            int rc = RBL_OK;
            int64_t k = 0;
            for (int64_t r0 = 0; r0 < n && rc == RBL_OK; r0 += chunk, ++k) {
                const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
                const int b = (int)(k & 1);
                const size_t bytes = ((size_t)(rows - 1) * (size_t)ldx + (size_t)ds) * esz;   // (the last row ends at column ds)
                hipError_t e = hipSuccess;
                if (k >= 2) e = hipStreamWaitEvent(copy_stream, formed[b], 0);   // staging buffer b has been consumed
                if (e == hipSuccess)
                    e = hipMemcpyAsync(Xd[b], (const unsigned char*)X + (size_t)r0 * (size_t)ldx * esz, bytes, hipMemcpyHostToDevice,
                                       copy_stream);
                if (e == hipSuccess) e = hipEventRecord(copied[b], copy_stream);
                if (e == hipSuccess) e = hipStreamWaitEvent(stream, copied[b], 0);
                if (e != hipSuccess) {
                    rbl_set_error("set_data_from: upload failed: %s", hipGetErrorString(e));
                    rc = RBL_ERR_HIP;
                    break;
                }
                rc = fn((const void*)Xd[b], r0, rows);
                if (rc == RBL_OK && hipEventRecord(formed[b], stream) != hipSuccess) rc = RBL_ERR_HIP;
            }
            if (hipStreamSynchronize(copy_stream) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
            return rc;
        });
    }
    // The CSR sibling: the same fn is handed dense rows.  Chunk by chunk the source's rows are expanded into the one
    // staging buffer (expansion and fn run on `stream`, in order) - a device source straight from the caller's arrays, a
    // host source from slices of the three arrays that the copy stream brings over one chunk ahead.
    // `sparse` (RBL_STORE_CSR): nothing is expanded - the chunk's slices of indices / values (entries [base, base + cnt) of
    // the source) go to sparse(indices, values, chunk, base, cnt) instead, and fn is not called.
    typedef std::function<int(const void*, const void*, const CsrChunk&, int64_t, int64_t)> SparseFn;
    int pass_csr(const CsrView& v, int64_t n, int64_t chunk, int num_cu, const std::function<int(const void*, int64_t, int64_t)>& fn,
                 double* ms = nullptr, const SparseFn* sparse = nullptr) {
        return timed(ms, [&]() {
            int rc = RBL_OK;
            const int64_t nk = csr_chunk_count(n, chunk);
            for (int64_t k = 0; k < nk && rc == RBL_OK; ++k) {
                const CsrChunk c = csr_chunk(v.ip, n, chunk, k);
                const int b = (int)(k & 1);
                if (v.mem == RBL_MEM_DEVICE && sparse) {
                    rc = (*sparse)(v.indices, v.values, c, 0, v.nnz);
                    continue;
                }
                if (v.mem == RBL_MEM_DEVICE) {
                    rc = launch_csr_expand(v.dtype, v.index_type, stage, v.ldc, c.rows, v.ds, (const unsigned char*)v.indptr + (size_t)c.r0 * v.isz,
                                           v.indices, v.values, 0, v.nnz, c.r0, v.err, num_cu, stream);
                    if (rc == RBL_OK) rc = fn((const void*)stage, c.r0, c.rows);
                    continue;
                }
                hipError_t e = hipSuccess;
                if (k >= 2) e = hipStreamWaitEvent(copy_stream, formed[b], 0);   // slices b have been expanded
                if (e == hipSuccess)
                    e = hipMemcpyAsync(ipd[b], (const unsigned char*)v.indptr + (size_t)c.r0 * v.isz, (size_t)(c.rows + 1) * v.isz,
                                       hipMemcpyHostToDevice, copy_stream);
                if (e == hipSuccess && c.cnt > 0)
                    e = hipMemcpyAsync(idx[b], (const unsigned char*)v.indices + (size_t)c.base * v.isz, (size_t)c.cnt * v.isz,
                                       hipMemcpyHostToDevice, copy_stream);
                if (e == hipSuccess && c.cnt > 0)
                    e = hipMemcpyAsync(val[b], (const unsigned char*)v.values + (size_t)c.base * v.esz, (size_t)c.cnt * v.esz,
                                       hipMemcpyHostToDevice, copy_stream);
                if (e == hipSuccess) e = hipEventRecord(copied[b], copy_stream);
                if (e == hipSuccess) e = hipStreamWaitEvent(stream, copied[b], 0);
                if (e != hipSuccess) {
                    rbl_set_error("set_data_csr: upload failed: %s", hipGetErrorString(e));
                    rc = RBL_ERR_HIP;
                    break;
                }
                if (sparse) {
                    rc = (*sparse)(idx[b], val[b], c, c.base, c.cnt);
                    if (rc == RBL_OK && hipEventRecord(formed[b], stream) != hipSuccess) rc = RBL_ERR_HIP;
                    continue;
                }
                rc = launch_csr_expand(v.dtype, v.index_type, stage, v.ldc, c.rows, v.ds, ipd[b], idx[b], val[b], c.base, c.cnt, c.r0,
                                       v.err, num_cu, stream);
                if (rc == RBL_OK && hipEventRecord(formed[b], stream) != hipSuccess) rc = RBL_ERR_HIP;
                if (rc == RBL_OK) rc = fn((const void*)stage, c.r0, c.rows);
            }
            if (copy_stream && hipStreamSynchronize(copy_stream) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
            return rc;
        });
    }
    // body() enqueues one pass; timed on the handle's stream, first kernel to last (host source: the copies it waits for in
    // between included); returns with the stream idle
    int timed(double* ms, const std::function<int()>& body) {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        if (ms && (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventRecord(t0, stream) != hipSuccess))
            ms = nullptr;
        int rc = body();
        if (ms && hipEventRecord(t1, stream) != hipSuccess) ms = nullptr;
        if (hipStreamSynchronize(stream) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
        float el = 0.f;
        if (ms && rc == RBL_OK && hipEventElapsedTime(&el, t0, t1) == hipSuccess) *ms = (double)el;
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (rc == RBL_ERR_HIP) {
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) rbl_set_error("set_data_from: %s", hipGetErrorString(e));
        }
        return rc;
    }
};

// the raw value at (r, c) of a CSR source, for a message: 0 for an implicit entry
static int csr_value_at(const CsrView& v, int64_t r, int64_t c, double* out) {
    *out = 0.0;
    const int64_t a = v.ip[r], len = v.ip[r + 1] - a;
    if (len <= 0) return RBL_OK;
    std::vector<unsigned char> ib((size_t)len * v.isz);
    const hipMemcpyKind kind = v.mem == RBL_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    RBL_HIP(hipMemcpy(ib.data(), (const unsigned char*)v.indices + (size_t)a * v.isz, ib.size(), kind));
    for (int64_t k = 0; k < len; ++k) {
        const int64_t ck = v.index_type == RBL_INDEX_I64 ? ((const int64_t*)ib.data())[k] : (int64_t)((const int32_t*)ib.data())[k];
        if (ck != c) continue;
        unsigned char tmp8[8] = {0};
        RBL_HIP(hipMemcpy(tmp8, (const unsigned char*)v.values + (size_t)(a + k) * v.esz, v.esz, kind));
        *out = src_host_widen(tmp8, v.dtype);
        break;
    }
    return RBL_OK;
}

// what the expand kernel refused, read after a pass: RBL_ERR_INVALID with the first offending entry of the smallest
// offending row (looked up in the source) in the message
static int csr_verdict(const CsrView& v) {
    u64 got[2] = {0ull, 0ull};
    RBL_HIP(hipMemcpy(got, v.err, sizeof(got), hipMemcpyDeviceToHost));
    if (got[0] == 0) return RBL_OK;
    const int64_t r = (int64_t)got[1], a = v.ip[r], len = v.ip[r + 1] - a;
    std::vector<unsigned char> ib((size_t)(len > 0 ? len : 1) * v.isz);
    RBL_HIP(hipMemcpy(ib.data(), (const unsigned char*)v.indices + (size_t)a * v.isz, (size_t)len * v.isz,
                      v.mem == RBL_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    static const char* fix = "canonical CSR is required: sort the indices of every row and sum duplicates first (SciPy: "
                             "sum_duplicates(); torch: coalesce() the COO tensor before to_sparse_csr())";
    int64_t prev = -1;
    for (int64_t k = 0; k < len; ++k) {
        const int64_t c = v.index_type == RBL_INDEX_I64 ? ((const int64_t*)ib.data())[k] : (int64_t)((const int32_t*)ib.data())[k];
        if (c < 0 || c >= v.ds) {
            rbl_set_error("set_data_csr: %llu entries refused, first in row %lld: column index %lld (entry %lld of the row) is "
                          "outside [0, %lld)", got[0], (long long)r, (long long)c, (long long)k, (long long)v.ds);
            return RBL_ERR_INVALID;
        }
        if (k > 0 && c == prev) {
            rbl_set_error("set_data_csr: %llu entries refused, first in row %lld: column index %lld is repeated (entries %lld "
                          "and %lld of the row) - duplicates are not summed; %s", got[0], (long long)r, (long long)c,
                          (long long)(k - 1), (long long)k, fix);
            return RBL_ERR_INVALID;
        }
        if (k > 0 && c < prev) {
            rbl_set_error("set_data_csr: %llu entries refused, first in row %lld: column index %lld follows %lld (entries %lld "
                          "and %lld of the row) - the indices of a row must be strictly increasing; %s", got[0], (long long)r,
                          (long long)c, (long long)prev, (long long)(k - 1), (long long)k, fix);
            return RBL_ERR_INVALID;
        }
        prev = c;
    }
    rbl_set_error("set_data_csr: %llu entries refused, first in row %lld (the arrays changed during the call?)", got[0],
                  (long long)r);
    return RBL_ERR_INVALID;
}

// cs == NULL: the dense source X / ldx.  cs != NULL: the CSR source *cs (X is NULL), expanded chunk by chunk into dense
// staging rows of stride cs->ldc that the same kernels read.
static int set_data_from_impl(rbl_solver* h, const void* X, int dtype, int mem, int64_t ldx, const double* y, int scaling,
                              int64_t ds, CsrView* cs = nullptr) {
    const int64_t n = h->n, d = h->d, ld = h->ld;
    const size_t esz = src_esz(dtype);
    {
        std::vector<signed char> ys((size_t)n);
        for (int64_t i = 0; i < n; ++i) ys[(size_t)i] = y[i] > 0 ? 1 : -1;
        RBL_HIP(hipMemcpy(h->ysign, ys.data(), (size_t)n, hipMemcpyHostToDevice));
    }
    SrcPipe p;
    p.stream = h->stream;
    h->src_ms[0] = h->src_ms[1] = 0.0;
    h->src_timed[0] = h->src_timed[1] = 0;
    const int64_t SB = src_stat_rows();
    int64_t chunk = n;
    long long cb = 64LL << 20;
    if (const char* e = getenv("RBL_UPLOAD_CHUNK_BYTES")) {   // test hook: several chunks at small sizes
        const long long v = atoll(e);
        if (v > 0) cb = v;
    }
    if (cs) {   // a device source is chunked as well: the dense staging buffer stays at chunk size
        cs->ldc = round_up(ds, (int64_t)(16 / esz));
        ldx = cs->ldc;
        chunk = csr_chunk_rows((int64_t)cb, (int64_t)(esz * (size_t)ldx), n, scaling == RBL_SCALE_FIT ? SB : 0);
        RBL_TRY(p.tmp.alloc(&p.stage, (size_t)chunk * (size_t)ldx * esz));
        RBL_TRY(p.tmp.alloc(&cs->err, 2));
        if (mem == RBL_MEM_HOST) {
            const size_t cap = (size_t)csr_max_chunk_nnz(cs->ip, n, chunk);
            p.pin(cs->indptr, (size_t)(n + 1) * cs->isz, 0);
            p.pin(cs->indices, (size_t)cs->nnz * cs->isz, 1);
            p.pin(cs->values, (size_t)cs->nnz * esz, 2);
            for (int b = 0; b < 2; ++b) {
                RBL_TRY(p.tmp.alloc(&p.ipd[b], (size_t)(chunk + 1) * cs->isz));
                RBL_TRY(p.tmp.alloc(&p.idx[b], cap * cs->isz));
                RBL_TRY(p.tmp.alloc(&p.val[b], cap * esz));
            }
            RBL_TRY(p.open_copy_stream());
        }
    } else if (mem == RBL_MEM_HOST) {
        chunk = (int64_t)(cb / (long long)(esz * (size_t)ldx));
        if (scaling == RBL_SCALE_FIT) {   // whole row blocks of the statistics (the other modes: 64 MB)
            chunk = chunk / SB * SB;
            if (chunk < SB) chunk = SB;
        }
        if (chunk < 1) chunk = 1;
        if (chunk > n) chunk = n;
        const size_t xbytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)ds) * esz;
        RBL_TRY(p.open_host(X, xbytes, (size_t)chunk * (size_t)ldx * esz));
    }
    const u64 pair0[2] = {0ull, ~0ull};   // {count, smallest position}
    // one pass over the source, whichever kind; a CSR source's entry checks are read when the pass has ended
    auto run_pass = [&](const std::function<int(const void*, int64_t, int64_t)>& fn, double* ms) -> int {
        if (!cs) return p.pass(X, mem, esz, ldx, ds, n, chunk, fn, ms);
        RBL_HIP(hipMemcpy(cs->err, pair0, sizeof(pair0), hipMemcpyHostToDevice));
        RBL_TRY(p.pass_csr(*cs, n, chunk, h->num_cu, fn, ms));
        return csr_verdict(*cs);
    };
    u64* ovf = nullptr;   // RBL_STORE_F16: {entries that do not fit, first of them} written by the forming kernel
    if (h->storage == RBL_STORE_F16) {
        RBL_TRY(p.tmp.alloc(&ovf, 2));
        RBL_HIP(hipMemcpy(ovf, pair0, sizeof(pair0), hipMemcpyHostToDevice));
    }
    double *dmean = nullptr, *dinv = nullptr;
    std::vector<double> fit_mean, fit_scale;   // RBL_SCALE_FIT: kept in the handle after the forming pass has succeeded
    if (scaling == RBL_SCALE_FIT) {
        const int64_t nb = (n + SB - 1) / SB;
        double *slab = nullptr, *shift = nullptr, *sums = nullptr;
        RBL_TRY(p.tmp.alloc(&slab, (size_t)nb * ld * 2));
        RBL_TRY(p.tmp.alloc(&shift, (size_t)ld));
        RBL_TRY(p.tmp.alloc(&sums, (size_t)ld * 2));
        RBL_HIP(hipMemsetAsync(slab, 0, sizeof(double) * (size_t)nb * ld * 2, h->stream));
        std::vector<double> sh((size_t)ld, 0.0), st((size_t)ld * 2, 0.0);
        if (cs) {   // row 0 expanded into the staging buffer (its refused entries are counted by the pass)
            const void *ipc = cs->indptr, *idc = cs->indices, *vlc = cs->values;
            const int64_t cnt0 = cs->ip[1];
            if (mem == RBL_MEM_HOST) {
                RBL_HIP(hipMemcpyAsync(p.ipd[0], cs->indptr, 2 * cs->isz, hipMemcpyHostToDevice, h->stream));
                if (cnt0 > 0) {
                    RBL_HIP(hipMemcpyAsync(p.idx[0], cs->indices, (size_t)cnt0 * cs->isz, hipMemcpyHostToDevice, h->stream));
                    RBL_HIP(hipMemcpyAsync(p.val[0], cs->values, (size_t)cnt0 * esz, hipMemcpyHostToDevice, h->stream));
                }
                ipc = p.ipd[0], idc = p.idx[0], vlc = p.val[0];
            }
            RBL_HIP(hipMemcpy(cs->err, pair0, sizeof(pair0), hipMemcpyHostToDevice));
            RBL_TRY(launch_csr_expand(dtype, cs->index_type, p.stage, ldx, 1, ds, ipc, idc, vlc, 0, cnt0, 0, cs->err, h->num_cu, h->stream));
            RBL_HIP(hipMemsetAsync(shift, 0, sizeof(double) * ld, h->stream));
            RBL_TRY(launch_src_row(dtype, p.stage, ds, shift, h->stream));
            RBL_HIP(hipStreamSynchronize(h->stream));
        } else if (mem == RBL_MEM_HOST) {   // the shift: the column's first row, widened
            for (int64_t j = 0; j < ds; ++j) sh[(size_t)j] = src_host_widen((const unsigned char*)X + (size_t)j * esz, dtype);
            RBL_HIP(hipMemcpyAsync(shift, sh.data(), sizeof(double) * ld, hipMemcpyHostToDevice, h->stream));
            RBL_HIP(hipStreamSynchronize(h->stream));
        } else {
            RBL_HIP(hipMemsetAsync(shift, 0, sizeof(double) * ld, h->stream));
            RBL_TRY(launch_src_row(dtype, X, ds, shift, h->stream));
        }
        double* slab2 = slab + (size_t)nb * ld;
        RBL_TRY(run_pass([&](const void* Xc, int64_t r0, int64_t rows) {
            return launch_src_colstats(dtype, Xc, ldx, rows, ds, shift, slab, slab2, ld, r0 / SB, h->stream);
        }, &h->src_ms[0]));
        h->src_timed[0] = 1;
        RBL_TRY(launch_src_colreduce(slab, nb, ld, sums, h->stream));
        RBL_TRY(launch_src_colreduce(slab2, nb, ld, sums + ld, h->stream));
        RBL_HIP(hipMemcpyAsync(st.data(), sums, sizeof(double) * ld * 2, hipMemcpyDeviceToHost, h->stream));
        RBL_HIP(hipMemcpyAsync(sh.data(), shift, sizeof(double) * ld, hipMemcpyDeviceToHost, h->stream));
        RBL_HIP(hipStreamSynchronize(h->stream));
        std::vector<double> mean((size_t)d, 0.0), scale((size_t)d, 1.0);
        const double nn = (double)n;
        for (int64_t j = 0; j < ds; ++j) {
            // x = shift + dl:  mean = shift + sum dl / n,  var = sum dl^2 / n - (sum dl / n)^2  (dl is of the size of the
            // column's spread, so nothing cancels against the column's mean)
            const double m1 = st[(size_t)j] / nn;
            const double mu = sh[(size_t)j] + m1;
            double var = st[(size_t)(ld + j)] / nn - m1 * m1;
            if (!std::isfinite(mu) || !std::isfinite(var)) {
                rbl_set_error("set_data_from: column %lld has a non-finite mean or variance (mean %g, variance %g) - the "
                              "source holds inf / nan or overflows fp64 sums", (long long)j, mu, var);
                return RBL_ERR_INVALID;
            }
            if (!(var > 0.0)) var = 1.0;   // a constant column is left at x - mean = 0
            mean[(size_t)j] = h->center ? mu : 0.0;   // (centring off: the same scale, the forming pass subtracts zero)
            scale[(size_t)j] = std::sqrt(var);
        }
        fit_mean.swap(mean);
        fit_scale.swap(scale);
    }
    if (scaling != RBL_SCALE_NONE) {
        const std::vector<double>& use_mean = scaling == RBL_SCALE_FIT ? fit_mean : h->sc_mean;
        const std::vector<double>& use_scale = scaling == RBL_SCALE_FIT ? fit_scale : h->sc_scale;
        std::vector<double> mi((size_t)ld * 2, 0.0);
        for (int64_t j = 0; j < ld; ++j) mi[(size_t)(ld + j)] = 1.0;
        for (int64_t j = 0; j < ds; ++j) {
            mi[(size_t)j] = use_mean[(size_t)j];
            mi[(size_t)(ld + j)] = 1.0 / use_scale[(size_t)j];
        }
        dmean = h->colstats + 2 * ld;
        dinv = h->colstats + 3 * ld;
        RBL_HIP(hipMemcpy(dmean, mi.data(), sizeof(double) * ld * 2, hipMemcpyHostToDevice));
    }
    RBL_TRY(run_pass([&](const void* Xc, int64_t r0, int64_t rows) {
        return launch_form_src(dtype, h->storage, h->D, ld, r0, Xc, ldx, h->ysign + r0, rows, ds, d, dmean, dinv, h->num_cu,
                               h->stream, ovf);
    }, &h->src_ms[1]));
    h->src_timed[1] = 1;
    if (ovf) {   // read once, after the last chunk
        u64 got[2] = {0ull, 0ull};
        RBL_HIP(hipMemcpy(got, ovf, sizeof(got), hipMemcpyDeviceToHost));
        if (got[0] > 0) {
            const long long r = (long long)(got[1] / (u64)d), c = (long long)(got[1] % (u64)d);
            double raw = 0.0;
            const unsigned char* at = (const unsigned char*)X + ((size_t)r * (size_t)ldx + (size_t)c) * esz;
            if (cs) {
                RBL_TRY(csr_value_at(*cs, r, c, &raw));
            } else if (mem == RBL_MEM_HOST) {
                raw = src_host_widen(at, dtype);
            } else {
                unsigned char tmp8[8] = {0};
                RBL_HIP(hipMemcpy(tmp8, at, esz, hipMemcpyDeviceToHost));
                raw = src_host_widen(tmp8, dtype);
            }
            rbl_set_error("fp16 storage: %llu finite entries do not fit float16 (|x| >= 65520), first at row %lld, column %lld "
                          "(value %g) - standardise the columns or use storage f32",
                          got[0], r, c, raw);
            return RBL_ERR_INVALID;
        }
    }
    if (scaling == RBL_SCALE_FIT) {   // the vectors are the handle's only once D stands: a failed call leaves the old ones
        h->sc_mean.swap(fit_mean);
        h->sc_scale.swap(fit_scale);
        h->sc_set = true;
    }
    return RBL_OK;
}

// RBL_STORE_CSR: the CSR source *cs becomes the handle's D as it comes - no dense chunk, no forming kernel.  The chunks,
// the pinned double-buffered copies of a host source and the verdict are those of the dense route; the entries go through
// launch_csr_store (spmv.hip), then the column form is built on the device.
// body() enqueues kernels on s; *ms += what they took (HIP events); returns with s idle
static int csr_timed(hipStream_t s, double* ms, const std::function<int()>& body) {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool on = hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess && hipEventRecord(t0, s) == hipSuccess;
    int rc = body();
    if (on && hipEventRecord(t1, s) != hipSuccess) on = false;
    if (hipStreamSynchronize(s) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;
    float el = 0.f;
    if (on && rc == RBL_OK && hipEventElapsedTime(&el, t0, t1) == hipSuccess) *ms += (double)el;
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (rc == RBL_ERR_HIP) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rbl_set_error("set_data_csr: %s", hipGetErrorString(e));
    }
    return rc;
}

// RBL_STORE_CSR with centring off: the entries stand unscaled in both forms (csr_store_finish has run).  RBL_SCALE_FIT
// takes the columns' statistics from the column form - two passes (spmv.hip: launch_csr_colstats), the mean of the
// shifted values formed on the host in between - then, as RBL_SCALE_APPLY does with the handle's vector, every stored
// value is multiplied by fl(1.0 / scale) of its column.  -y_r x is exact, so scaling the stored values has the bits of
// scaling at store time; both modes scale after the store.  The column of ones is never scaled (mean 0, scale 1).
static int csr_scale_only(rbl_solver* h, CsrStore* st, int64_t ds, int scaling) {
    const int64_t n = h->n, d = h->d, ld = h->ld;
    DevArena tmp;   // freed on return: every launch below is waited for
    double* dinv = nullptr;
    RBL_TRY(tmp.alloc(&dinv, (size_t)ld));
    std::vector<double> fit_scale;
    if (scaling == RBL_SCALE_FIT) {
        double *part = nullptr, *sums = nullptr, *mud = nullptr;
        RBL_TRY(tmp.alloc(&part, (size_t)st->nseg));
        RBL_TRY(tmp.alloc(&sums, (size_t)ld));
        RBL_TRY(tmp.alloc(&mud, (size_t)ld));
        std::vector<double> s1((size_t)ld, 0.0), s2((size_t)ld, 0.0), m1((size_t)ld, 0.0);
        std::vector<int64_t> cp((size_t)ld + 1, 0);
        const double nn = (double)n;
        RBL_TRY(csr_timed(h->stream, &h->src_ms[0], [&]() {
            return launch_csr_colstats(st, n, ld, h->ysign, 1, nullptr, part, sums, h->num_cu, h->stream);
        }));
        RBL_HIP(hipMemcpy(s1.data(), sums, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost));
        RBL_HIP(hipMemcpy(cp.data(), st->colptr, sizeof(int64_t) * (size_t)(ld + 1), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < ds; ++j) m1[(size_t)j] = s1[(size_t)j] / nn;
        RBL_HIP(hipMemcpy(mud, m1.data(), sizeof(double) * (size_t)ld, hipMemcpyHostToDevice));
        RBL_TRY(csr_timed(h->stream, &h->src_ms[0], [&]() {
            return launch_csr_colstats(st, n, ld, h->ysign, 2, mud, part, sums, h->num_cu, h->stream);
        }));
        h->src_timed[0] = 1;
        RBL_HIP(hipMemcpy(s2.data(), sums, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost));
        fit_scale.assign((size_t)d, 1.0);
        for (int64_t j = 0; j < ds; ++j) {
            // x = sh + dl over the stored entries, 0 over the n - cnt others (sh = 0 unless the column is full):
            // mean = sh + m1, m1 = sum dl / n;  var = (sum (dl - m1)^2 + (n - cnt) m1^2) / n
            const double mu = m1[(size_t)j], rest = (double)(n - (cp[(size_t)j + 1] - cp[(size_t)j]));
            double var = (s2[(size_t)j] + rest * (mu * mu)) / nn;
            if (!std::isfinite(mu) || !std::isfinite(var)) {
                rbl_set_error("set_data_csr: column %lld has a non-finite mean or variance (shifted mean %g, variance %g) - the "
                              "source holds inf / nan or overflows fp64 sums", (long long)j, mu, var);
                return RBL_ERR_INVALID;
            }
            if (!(var > 0.0)) var = 1.0;   // a constant column keeps its values
            fit_scale[(size_t)j] = std::sqrt(var);
        }
    }
    const std::vector<double>& use = scaling == RBL_SCALE_FIT ? fit_scale : h->sc_scale;
    std::vector<double> inv((size_t)ld, 1.0);
    for (int64_t j = 0; j < ds; ++j) inv[(size_t)j] = 1.0 / use[(size_t)j];
    RBL_HIP(hipMemcpy(dinv, inv.data(), sizeof(double) * (size_t)ld, hipMemcpyHostToDevice));
    RBL_TRY(csr_timed(h->stream, &h->src_ms[1], [&]() { return launch_csr_scale(st, ld, dinv, h->num_cu, h->stream); }));
    if (scaling == RBL_SCALE_FIT) {   // the vectors are the handle's only once D stands
        h->sc_mean.assign((size_t)d, 0.0);
        h->sc_scale.swap(fit_scale);
        h->sc_set = true;
    }
    return RBL_OK;
}

static int set_data_csr_sparse(rbl_solver* h, const double* y, int64_t ds, int ones, CsrView* cs, int scaling) {
    const int64_t n = h->n, ld = h->ld;
    CsrStore* st = (CsrStore*)h->D;
    st->lanes = 0;
    {
        std::vector<signed char> ys((size_t)n);
        for (int64_t i = 0; i < n; ++i) ys[(size_t)i] = y[i] > 0 ? 1 : -1;
        RBL_HIP(hipMemcpy(h->ysign, ys.data(), (size_t)n, hipMemcpyHostToDevice));
    }
    // nothing reads the entry buffers while they are regrown (data_write_begins has waited for the borrowers).  A borrower's
    // slab follows the new segment count at its next q pass (api_iter.hip)
    RBL_HIP(hipStreamSynchronize(h->stream));
    const bool columns = !h->cfg.objective_only;
    RBL_TRY(csr_store_reserve(*h->shared, st, n, ld, cs->nnz + (ones ? n : 0), columns));
    {   // D's own indptr: the source's, plus one slot per row with the column of ones
        std::vector<int64_t> op((size_t)n + 1);
        for (int64_t r = 0; r <= n; ++r) op[(size_t)r] = cs->ip[r] + (ones ? r : 0);
        RBL_HIP(hipMemcpy(st->indptr, op.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
        st->pair_products = csr_gram_pair_products(op.data(), n, 0);   // what G from the entries costs (csr_gram_plan.h)
    }
    SrcPipe p;
    p.stream = h->stream;
    h->src_ms[0] = h->src_ms[1] = 0.0;
    h->src_timed[0] = h->src_timed[1] = 0;
    long long cb = 64LL << 20;
    if (const char* e = getenv("RBL_UPLOAD_CHUNK_BYTES")) {   // test hook: several chunks at small sizes
        const long long v = atoll(e);
        if (v > 0) cb = v;
    }
    // rows of a chunk: as many as an average row's share of the source arrays fits the chunk size
    const int64_t per_row = (int64_t)cs->isz + (int64_t)(cs->isz + cs->esz) * ((cs->nnz + n - 1) / n);
    const int64_t chunk = csr_chunk_rows((int64_t)cb, per_row, n, 0);
    RBL_TRY(p.tmp.alloc(&cs->err, 2));
    if (cs->mem == RBL_MEM_HOST) {
        const size_t cap = (size_t)csr_max_chunk_nnz(cs->ip, n, chunk);
        p.pin(cs->indptr, (size_t)(n + 1) * cs->isz, 0);
        p.pin(cs->indices, (size_t)cs->nnz * cs->isz, 1);
        p.pin(cs->values, (size_t)cs->nnz * cs->esz, 2);
        for (int b = 0; b < 2; ++b) {
            RBL_TRY(p.tmp.alloc(&p.ipd[b], (size_t)(chunk + 1) * cs->isz));
            RBL_TRY(p.tmp.alloc(&p.idx[b], cap * cs->isz));
            RBL_TRY(p.tmp.alloc(&p.val[b], cap * cs->esz));
        }
        RBL_TRY(p.open_copy_stream());
    }
    const u64 pair0[2] = {0ull, ~0ull};   // {count, smallest position}
    RBL_HIP(hipMemcpy(cs->err, pair0, sizeof(pair0), hipMemcpyHostToDevice));
    const SrcPipe::SparseFn store = [&](const void* idx, const void* val, const CsrChunk& c, int64_t base, int64_t cnt) {
        return launch_csr_store(cs->dtype, cs->index_type, st, c.rows, c.r0, ds, ones, idx, val, base, cnt, h->ysign, cs->err,
                                h->num_cu, h->stream);
    };
    RBL_TRY(p.pass_csr(*cs, n, chunk, h->num_cu, nullptr, &h->src_ms[1], &store));
    h->src_timed[1] = 1;
    RBL_TRY(csr_verdict(*cs));
    RBL_TRY(csr_store_finish(st, ld, columns, h->num_cu, h->stream));
    if (scaling != RBL_SCALE_NONE) {   // centring off (the entry point has refused everything else)
        const int rc = csr_scale_only(h, st, ds, scaling);
        if (rc != RBL_OK) st->lanes = 0;   // the values are not what the call promised: nothing reads them
        RBL_TRY(rc);
    }
    return RBL_OK;   // (the slab of the q pass follows the segment count where the pass is launched: api_iter.hip)
}

// In front of every write to D or the labels beside it: the data epoch moves, so that whoever holds something computed
// from the old D - this handle, its borrowers - drops it (sync_data_epoch), whether the write completes or not.  With
// borrowers, each on a stream of its own, the whole device is waited for: no pass of theirs still streams what is
// overwritten (dense storage) or freed and regrown (sparse storage).  A handle on its own never pays that wait.
static int data_write_begins(rbl_solver* h) {
    h->sd->epoch += 1;
    h->sd->complete = false;
    if (h->shared.use_count() > 1) RBL_HIP(hipDeviceSynchronize());
    return RBL_OK;
}

// ... and behind it, once D stands
static int data_written(rbl_solver* h) {
    h->data_ready = true;
    h->sd->complete = true;
    data_changed(h->der);
    h->epoch = h->sd->epoch;
    return RBL_OK;
}

// what a handle with RBL_STORE_CSR takes no part in (`who`: the entry point): RBL_ERR_INVALID, the handle without data
static int refuse_on_csr(rbl_solver* h, const char* who, const char* why) {
    if (h->storage != RBL_STORE_CSR) return RBL_OK;
    if (!h->borrower) h->data_ready = false;
    rbl_set_error("%s: %s", who, why);
    return RBL_ERR_INVALID;
}

// labels are +1 / -1, nothing else (`who`: the entry point's name in the message)
static int check_labels(const char* who, const double* y, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(y[i] == 1.0 || y[i] == -1.0)) {
            rbl_set_error("%s: labels must be +1/-1 (y[%lld] = %g)", who, (long long)i, y[i]);
            return RBL_ERR_INVALID;
        }
    return RBL_OK;
}

// the argument checks the dense and the CSR entry share (`who`: the entry point's name in the message)
static int check_source_args(rbl_solver* h, const char* who, int dtype, int mem, int scaling, int flags) {
    if (dtype != RBL_DTYPE_F64 && dtype != RBL_DTYPE_F32 && dtype != RBL_DTYPE_F16) {
        rbl_set_error("%s: unknown dtype %d (RBL_DTYPE_F64 / F32 / F16)", who, dtype);
        return RBL_ERR_INVALID;
    }
    if (mem != RBL_MEM_HOST && mem != RBL_MEM_DEVICE) {
        rbl_set_error("%s: unknown memory kind %d (RBL_MEM_HOST / RBL_MEM_DEVICE)", who, mem);
        return RBL_ERR_INVALID;
    }
    if (scaling != RBL_SCALE_NONE && scaling != RBL_SCALE_FIT && scaling != RBL_SCALE_APPLY) {
        rbl_set_error("%s: unknown scaling %d (RBL_SCALE_NONE / FIT / APPLY)", who, scaling);
        return RBL_ERR_INVALID;
    }
    if (flags & ~RBL_DATA_ONES_COLUMN) {
        rbl_set_error("%s: unknown flags 0x%x", who, (unsigned)flags);
        return RBL_ERR_INVALID;
    }
    return RBL_OK;
}
static int check_scaling_state(rbl_solver* h, const char* who, int scaling) {
    if (scaling == RBL_SCALE_FIT && h->nt != h->n) {
        rbl_set_error("%s: RBL_SCALE_FIT on a row-sharded handle (n = %lld of n_total = %lld) - reduce the column "
                      "sums over the ranks in the driver, hand every rank the same vectors (rbl_set_scaling) and use "
                      "RBL_SCALE_APPLY", who, (long long)h->n, (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    if (scaling == RBL_SCALE_FIT && h->n < 1) {
        rbl_set_error("%s: RBL_SCALE_FIT needs at least one row", who);
        return RBL_ERR_INVALID;
    }
    if (scaling == RBL_SCALE_APPLY && !h->sc_set) {
        rbl_set_error("%s: RBL_SCALE_APPLY without a scaling - call rbl_set_scaling first", who);
        return RBL_ERR_STATE;
    }
    if (scaling == RBL_SCALE_APPLY && !h->center)
        for (int64_t j = 0; j < h->d; ++j)
            if (h->sc_mean[(size_t)j] != 0.0) {
                rbl_set_error("%s: RBL_SCALE_APPLY with centring off (rbl_set_centering) takes an all-zero mean vector, mean[%lld] "
                              "is %g - these vectors come from a centred fit: turn centring on, or set the means to zero", who,
                              (long long)j, h->sc_mean[(size_t)j]);
                return RBL_ERR_INVALID;
            }
    return RBL_OK;
}

extern "C" {

int rbl_set_data_from(rbl_solver* h, const void* X, int dtype, int mem, int64_t ldx, const double* y, int scaling, int flags) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "set_data_from");
    RBL_TRY(check_source_args(h, "set_data_from", dtype, mem, scaling, flags));
    RBL_TRY(refuse_on_csr(h, "set_data_from", "a dense source on a handle with RBL_STORE_CSR - sparse storage takes its data "
                                               "through rbl_set_data_csr (a dense matrix belongs in storage f32 / f64 / fp16)"));
    const int64_t n = h->n, d = h->d;
    const int64_t ds = d - ((flags & RBL_DATA_ONES_COLUMN) ? 1 : 0);
    if (!X || !y || ds < 1 || ldx < ds) {
        rbl_set_error("set_data_from: bad arguments (X %s, y %s, ldx=%lld, source columns=%lld)", X ? "given" : "NULL",
                      y ? "given" : "NULL", (long long)ldx, (long long)ds);
        return RBL_ERR_INVALID;
    }
    if ((size_t)(uintptr_t)X % src_esz(dtype) != 0) {
        rbl_set_error("set_data_from: X is not aligned to its element size (%zu bytes)", src_esz(dtype));
        return RBL_ERR_INVALID;
    }
    RBL_TRY(check_labels("set_data_from", y, n));
    RBL_TRY(check_scaling_state(h, "set_data_from", scaling));
    if (n > 0) {
        if (mem == RBL_MEM_DEVICE)
            RBL_TRY(src_check_device_range(X, ((size_t)(n - 1) * (size_t)ldx + (size_t)ds) * src_esz(dtype), h->cfg.device));
        h->data_ready = false;   // a failed upload leaves the handle without data
        RBL_TRY(data_write_begins(h));
        RBL_TRY(set_data_from_impl(h, X, dtype, mem, ldx, y, scaling, ds));
    }
    return data_written(h);
}

int rbl_set_data_csr(rbl_solver* h, const void* indptr, const void* indices, const void* values, int64_t nnz, int index_type,
                     int dtype, int mem, const double* y, int scaling, int flags) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "set_data_csr");
    RBL_TRY(check_source_args(h, "set_data_csr", dtype, mem, scaling, flags));
    if (index_type != RBL_INDEX_I32 && index_type != RBL_INDEX_I64) {
        rbl_set_error("set_data_csr: unknown index type %d (RBL_INDEX_I32 / RBL_INDEX_I64)", index_type);
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n, d = h->d;
    const int64_t ds = d - ((flags & RBL_DATA_ONES_COLUMN) ? 1 : 0);
    if (h->storage == RBL_STORE_CSR) {
        if (scaling != RBL_SCALE_NONE && h->center)
            return refuse_on_csr(h, "set_data_csr", "RBL_SCALE_FIT / RBL_SCALE_APPLY on a handle with RBL_STORE_CSR - centring the "
                                                    "columns makes D dense; scale the source yourself or use a dense storage type");
        if (scaling == RBL_SCALE_FIT && h->cfg.objective_only)
            return refuse_on_csr(h, "set_data_csr", "RBL_SCALE_FIT on an objective-only handle with RBL_STORE_CSR - the column "
                                                    "statistics are taken from the column form, which such a handle does not "
                                                    "build; give it the training vectors (rbl_set_scaling) and use RBL_SCALE_APPLY");
        if (nnz > 0x7fffffffLL || (nnz >= 0 && nnz + ((flags & RBL_DATA_ONES_COLUMN) ? n : 0) > 0x7fffffffLL)) {   // (n <= 2^31 - 1)
            char why[256];
            snprintf(why, sizeof(why), "nnz = %lld%s exceeds the 2^31 - 1 entries a handle with RBL_STORE_CSR holds", (long long)nnz,
                     (flags & RBL_DATA_ONES_COLUMN) ? " (plus n for the column of ones)" : "");
            return refuse_on_csr(h, "set_data_csr", why);
        }
    }
    if (!indptr || !y || ds < 1 || nnz < 0 || (nnz > 0 && (!indices || !values))) {
        rbl_set_error("set_data_csr: bad arguments (indptr %s, indices %s, values %s, y %s, nnz=%lld, source columns=%lld)",
                      indptr ? "given" : "NULL", indices ? "given" : "NULL", values ? "given" : "NULL", y ? "given" : "NULL",
                      (long long)nnz, (long long)ds);
        return RBL_ERR_INVALID;
    }
    CsrView v;
    v.indptr = indptr, v.indices = nnz ? indices : nullptr, v.values = nnz ? values : nullptr;
    v.nnz = nnz, v.index_type = index_type, v.dtype = dtype, v.mem = mem, v.ds = ds;
    v.isz = index_type == RBL_INDEX_I64 ? 8 : 4, v.esz = src_esz(dtype);
    if ((size_t)(uintptr_t)indptr % v.isz != 0 || (size_t)(uintptr_t)v.indices % v.isz != 0 || (size_t)(uintptr_t)v.values % v.esz != 0) {
        rbl_set_error("set_data_csr: indptr / indices / values are not aligned to their element sizes (%zu / %zu / %zu bytes)",
                      v.isz, v.isz, v.esz);
        return RBL_ERR_INVALID;
    }
    RBL_TRY(check_labels("set_data_csr", y, n));
    RBL_TRY(check_scaling_state(h, "set_data_csr", scaling));
    if (mem == RBL_MEM_DEVICE) {
        RBL_TRY(src_check_device_range(indptr, (size_t)(n + 1) * v.isz, h->cfg.device, "set_data_csr", "indptr"));
        if (nnz > 0) {
            RBL_TRY(src_check_device_range(indices, (size_t)nnz * v.isz, h->cfg.device, "set_data_csr", "indices"));
            RBL_TRY(src_check_device_range(values, (size_t)nnz * v.esz, h->cfg.device, "set_data_csr", "values"));
        }
    }
    // the structure of indptr, on the host, before anything is enqueued: a device indptr is copied once, and the 64-bit
    // copy plans the chunks
    std::vector<int64_t> ip((size_t)n + 1);
    {
        std::vector<unsigned char> raw;
        const void* src = indptr;
        if (mem == RBL_MEM_DEVICE) {
            raw.resize((size_t)(n + 1) * v.isz);
            RBL_HIP(hipStreamSynchronize(h->stream));
            RBL_HIP(hipMemcpy(raw.data(), indptr, raw.size(), hipMemcpyDeviceToHost));
            src = raw.data();
        }
        int64_t row = 0, got = 0;
        int bad;
        if (index_type == RBL_INDEX_I64) {
            bad = csr_check_indptr((const int64_t*)src, n, nnz, &row, &got);
            csr_widen_indptr((const int64_t*)src, n, ip.data());
        } else {
            bad = csr_check_indptr((const int32_t*)src, n, nnz, &row, &got);
            csr_widen_indptr((const int32_t*)src, n, ip.data());
        }
        if (bad == CSR_PLAN_FIRST) rbl_set_error("set_data_csr: indptr[0] is %lld, not 0", (long long)got);
        if (bad == CSR_PLAN_DECREASING)
            rbl_set_error("set_data_csr: indptr decreases at row %lld (indptr[%lld] = %lld < indptr[%lld] = %lld)", (long long)row,
                          (long long)(row + 1), (long long)got, (long long)row, (long long)ip[(size_t)row]);
        if (bad == CSR_PLAN_LAST)
            rbl_set_error("set_data_csr: indptr[n] is %lld, nnz is %lld (n = %lld rows)", (long long)got, (long long)nnz, (long long)n);
        if (bad != CSR_PLAN_OK) return RBL_ERR_INVALID;
    }
    v.ip = ip.data();
    if (n > 0) {
        h->data_ready = false;   // a failed upload leaves the handle without data
        RBL_TRY(data_write_begins(h));
        if (h->storage == RBL_STORE_CSR) RBL_TRY(set_data_csr_sparse(h, y, ds, (flags & RBL_DATA_ONES_COLUMN) ? 1 : 0, &v, scaling));
        else RBL_TRY(set_data_from_impl(h, nullptr, dtype, mem, 0, y, scaling, ds, &v));
    }
    return data_written(h);
}

// the float64 host route is the typed one (include/rbl.h)
int rbl_set_data(rbl_solver* h, const double* X, const double* y, int64_t ldx) {
    return rbl_set_data_from(h, X, RBL_DTYPE_F64, RBL_MEM_HOST, ldx, y, RBL_SCALE_NONE, 0);
}

int rbl_set_scaling(rbl_solver* h, const double* mean, const double* scale) {
    RBL_ENTER(h);
    if (!mean && !scale) {
        h->sc_mean.clear();
        h->sc_scale.clear();
        h->sc_set = false;
        return RBL_OK;
    }
    if (!mean || !scale) {
        rbl_set_error("set_scaling: mean and scale go together (both NULL clears them)");
        return RBL_ERR_INVALID;
    }
    for (int64_t j = 0; j < h->d; ++j) {
        if (!std::isfinite(mean[j]) || !std::isfinite(scale[j]) || !(scale[j] > 0.0)) {
            rbl_set_error("set_scaling: column %lld: mean %g / scale %g (finite values, scale > 0)", (long long)j, mean[j], scale[j]);
            return RBL_ERR_INVALID;
        }
    }
    h->sc_mean.assign(mean, mean + h->d);
    h->sc_scale.assign(scale, scale + h->d);
    h->sc_set = true;
    return RBL_OK;
}

int rbl_set_centering(rbl_solver* h, int center) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "set_centering");
    if (center != 0 && center != 1) {
        rbl_set_error("set_centering: center must be 0 or 1 (got %d)", center);
        return RBL_ERR_INVALID;
    }
    h->center = center != 0;
    return RBL_OK;
}

int rbl_get_centering(rbl_solver* h, int* center) {
    RBL_ENTER_ITER(h);
    if (center) *center = h->center ? 1 : 0;
    return RBL_OK;
}

int rbl_get_scaling(rbl_solver* h, double* mean, double* scale, int* is_set) {
    RBL_ENTER_ITER(h);
    for (int64_t j = 0; j < h->d; ++j) {
        if (mean) mean[j] = h->sc_set ? h->sc_mean[(size_t)j] : 0.0;
        if (scale) scale[j] = h->sc_set ? h->sc_scale[(size_t)j] : 1.0;
    }
    if (is_set) *is_set = h->sc_set ? 1 : 0;
    return RBL_OK;
}

int rbl_synth_local(rbl_solver* h, uint64_t seed, double class_sep, double flip_y) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "synth_local");
    RBL_TRY(refuse_on_csr(h, "synth_local", "the synthetic generator writes a dense matrix - not available with RBL_STORE_CSR"));
    // positions of the 2 informative + 2 redundant columns, the 2x2 mixing matrix of the redundant ones, the four
    // clusters' covariance matrices A_k (entries uniform in (-1, 1)) and which hypercube vertex each cluster sits on
    // (a random permutation; cluster k belongs to class k % 2) - make_classification's geometry draws - from a small
    // host-side LCG keyed by the seed (identical on every rank)
    uint64_t st = seed * 6364136223846793005ull + 1442695040888963407ull;
    auto next = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(st >> 33);
    };
    int special[4] = {-1, -1, -1, -1};
    const int nspec = h->d >= 4 ? 4 : (int)h->d;
    for (int k = 0; k < nspec; ++k) {
        for (;;) {
            int c = (int)(next() % (uint32_t)h->d);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= special[j] == c;
            if (!dup) {
                special[k] = c;
                break;
            }
        }
    }
    double mix[4];
    for (int k = 0; k < 4; ++k) mix[k] = 2.0 * ((double)next() / 2147483648.0) - 1.0;
    double A16[16];
    for (int k = 0; k < 16; ++k) A16[k] = 2.0 * ((double)next() / 2147483648.0) - 1.0;
    int vertex[4] = {0, 1, 2, 3};
    for (int i = 3; i > 0; --i) {
        const int j = (int)(next() % (uint32_t)(i + 1));
        std::swap(vertex[i], vertex[j]);
    }
    RBL_TRY(data_write_begins(h));   // (the labels now; D here or, fp16 storage, in rbl_synth_finish)
    if (h->storage == RBL_STORE_F16) {
        // the statistics of the unrounded draws; the matrix itself is written by rbl_synth_finish, in one rounding
        h->synth.pending = true;
        h->synth.seed = seed;
        h->synth.class_sep = class_sep;
        h->synth.flip_y = flip_y;
        for (int k = 0; k < 4; ++k) {
            h->synth.special[k] = special[k];
            h->synth.vertex[k] = vertex[k];
            h->synth.mix[k] = mix[k];
        }
        for (int k = 0; k < 16; ++k) h->synth.A16[k] = A16[k];
        h->data_ready = false;
        RBL_TRY(launch_synth_stats(h->n, h->ld, h->d, h->off, seed, class_sep, flip_y, special, mix, A16, vertex, h->ysign, h->slab,
                                   h->colstats, h->colstats + h->ld, h->num_cu, h->stream));
        RBL_HIP(hipStreamSynchronize(h->stream));
        return RBL_OK;
    }
    RBL_TRY(launch_synth(h->storage, h->D, h->n, h->ld, h->d, h->off, seed, class_sep, flip_y, special, mix, A16, vertex,
                         h->ysign, h->stream));
    // column sums / sums of squares of the local rows -> colstats[0 .. 2 ld)
    RBL_TRY(launch_colstats(h->storage, h->D, h->n, h->ld, h->slab, h->colstats, h->colstats + h->ld, h->num_cu,
                            h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    return RBL_OK;
}

int rbl_synth_finish(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "synth_finish");
    RBL_TRY(refuse_on_csr(h, "synth_finish", "the synthetic generator writes a dense matrix - not available with RBL_STORE_CSR"));
    // preprocessing.scale (load_data.py:115): (x - mean) / std with the population std
    const int64_t ld = h->ld;
    std::vector<double> st((size_t)ld * 4, 0.0);
    RBL_HIP(hipMemcpy(st.data(), h->colstats, sizeof(double) * ld * 2, hipMemcpyDeviceToHost));
    const double nt = (double)h->nt;
    for (int64_t j = 0; j < ld; ++j) {
        const double mean = st[j] / nt;
        double var = st[ld + j] / nt - mean * mean;
        if (!(var > 0.0)) var = 1.0;
        st[2 * ld + j] = mean;
        st[3 * ld + j] = 1.0 / std::sqrt(var);
    }
    RBL_HIP(hipMemcpy(h->colstats + 2 * ld, st.data() + 2 * ld, sizeof(double) * ld * 2, hipMemcpyHostToDevice));
    if (h->storage == RBL_STORE_F16) {
        if (!h->synth.pending) {
            rbl_set_error("synth_finish: call rbl_synth_local first");
            return RBL_ERR_STATE;
        }
        RBL_TRY(launch_synth_f16(h->D, h->n, ld, h->d, h->off, h->synth.seed, h->synth.class_sep, h->synth.flip_y, h->synth.special,
                                 h->synth.mix, h->synth.A16, h->synth.vertex, h->colstats + 2 * ld, h->colstats + 3 * ld, h->stream));
        h->synth.pending = false;
    } else {
        RBL_TRY(launch_standardize_negy(h->storage, h->D, h->n, ld, h->d, h->colstats + 2 * ld, h->colstats + 3 * ld,
                                        h->ysign, h->stream));
    }
    RBL_HIP(hipStreamSynchronize(h->stream));
    return data_written(h);
}

int rbl_generate_synthetic(rbl_solver* h, uint64_t seed, double class_sep, double flip_y) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "generate_synthetic");
    RBL_TRY(refuse_on_csr(h, "generate_synthetic", "the synthetic generator writes a dense matrix - not available with RBL_STORE_CSR"));
    if (h->nt != h->n) {
        rbl_set_error("generate_synthetic: sharded problem - use rbl_synth_local, sum RBL_BUF_COLSTATS, rbl_synth_finish");
        return RBL_ERR_STATE;
    }
    RBL_TRY(rbl_synth_local(h, seed, class_sep, flip_y));
    return rbl_synth_finish(h);
}

int rbl_set_penalty(rbl_solver* h, const double* l1, const double* l2) {
    RBL_ENTER(h);
    if (h->iter > 0) {
        rbl_set_error("set_penalty: the handle has iterated already (iter = %lld)", (long long)h->iter);
        return RBL_ERR_STATE;
    }
    if (!l1 && !l2) {
        rbl_set_error("set_penalty: l1 and l2 are both NULL");
        return RBL_ERR_INVALID;
    }
    if (!h->cfg.objective_only && h->cfg.wstep == RBL_WSTEP_SMOOTH_L1) {
        rbl_set_error("set_penalty: the smoothed-l1 w-step (sADMM) has no per-coordinate penalties");
        return RBL_ERR_INVALID;
    }
    const int64_t d = h->d, ld = h->ld;
    for (int k = 0; k < 2; ++k) {
        const double* v = k ? l2 : l1;
        for (int64_t j = 0; v && j < d; ++j)
            if (!(v[j] >= 0.0) || !std::isfinite(v[j])) {
                rbl_set_error("set_penalty: %s[%lld] = %g - penalties must be finite and >= 0", k ? "l2" : "l1", (long long)j,
                              v[j]);
                return RBL_ERR_INVALID;
            }
    }
    std::vector<double> host((size_t)(2 * ld + 8), 0.0);
    double l2max = 0.0;
    for (int64_t j = 0; j < d; ++j) {
        if (l1) host[(size_t)j] = l1[j];
        if (l2) {
            host[(size_t)(ld + j)] = l2[j];
            if (l2[j] > l2max) l2max = l2[j];
        }
    }
    if (!h->pen) RBL_TRY(h->mem.alloc(&h->pen, (size_t)(2 * ld + 8)));
    RBL_HIP(hipMemcpyAsync(h->pen, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, h->stream));
    RBL_HIP(hipStreamSynchronize(h->stream));
    h->pen_host.assign((size_t)(2 * d), 0.0);
    for (int64_t j = 0; j < d; ++j) {
        h->pen_host[(size_t)j] = host[(size_t)j];
        h->pen_host[(size_t)(d + j)] = host[(size_t)(ld + j)];
    }
    h->ww.pen_l1 = h->pen;
    h->ww.pen_l2 = h->pen + ld;
    h->ww.pen_l2max = l2max;
    if (h->wset) h->wset->built = false;   // which coordinates are free may have changed: the working set is built again
    return RBL_OK;
}

int rbl_get_penalty(rbl_solver* h, double* l1, double* l2, int* is_set) {
    RBL_ENTER_ITER(h);
    const int64_t d = h->d;
    if (is_set) *is_set = h->pen ? 1 : 0;
    for (int64_t j = 0; j < d; ++j) {
        if (l1) l1[j] = h->pen ? h->pen_host[(size_t)j] : 0.0;
        if (l2) l2[j] = h->pen ? h->pen_host[(size_t)(d + j)] : 0.0;
    }
    return RBL_OK;
}

int rbl_set_labels(rbl_solver* h, const double* y) {
    RBL_ENTER(h);
    if (!h->borrower) {
        rbl_set_error("set_labels: only a handle that borrows its data (rbl_create_shared) can carry labels of its own");
        return RBL_ERR_STATE;
    }
    if (h->iter > 0) {
        rbl_set_error("set_labels: the handle has iterated already (iter = %lld)", (long long)h->iter);
        return RBL_ERR_STATE;
    }
    if (h->in_group) {
        rbl_set_error("set_labels: the handle is a member of a group - destroy the group first");
        return RBL_ERR_STATE;
    }
    if (h->nt != h->n) {
        rbl_set_error("set_labels: row-sharded handle (n=%lld of %lld) - the distributed z-steps carry no labels of their own",
                      (long long)h->n, (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    if (!y) {
        rbl_set_error("set_labels: y is NULL");
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n;
    RBL_TRY(check_labels("set_labels", y, n));
    RBL_HIP(hipStreamSynchronize(h->stream));
    std::vector<signed char> yo((size_t)n), r((size_t)n), ys((size_t)n);
    RBL_HIP(hipMemcpy(yo.data(), h->ysign, (size_t)n, hipMemcpyDeviceToHost));
    bool differs = false;
    for (int64_t i = 0; i < n; ++i) {
        ys[(size_t)i] = y[i] > 0 ? 1 : -1;
        r[(size_t)i] = (signed char)(ys[(size_t)i] * yo[(size_t)i]);
        differs = differs || r[(size_t)i] < 0;
    }
    if (!differs && !h->rs) return RBL_OK;   // the owner's labels on an ordinary borrower: nothing changes
    // z and lambda move from the sign convention they are stored in to the new one (both start as constants)
    std::vector<double> zh, lh;
    if (h->z) {
        zh.resize((size_t)n);
        lh.resize((size_t)n);
        RBL_HIP(hipMemcpy(zh.data(), h->z, sizeof(double) * n, hipMemcpyDeviceToHost));
        RBL_HIP(hipMemcpy(lh.data(), h->lam, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (h->rs) {
            flip_rows(h, zh.data());
            flip_rows(h, lh.data());
        }
    }
    if (!differs) {   // the owner's labels: an ordinary borrower
        if (h->rs) h->mem.release(h->rs);
        h->rs = nullptr;
        h->rs_host.clear();
        h->ys_host.clear();
    } else {
        if (!h->rs) RBL_TRY(h->mem.alloc(&h->rs, (size_t)n));
        RBL_HIP(hipMemcpy(h->rs, r.data(), (size_t)n, hipMemcpyHostToDevice));
        h->rs_host.swap(r);
        h->ys_host.swap(ys);
    }
    if (h->z) {
        RBL_TRY(upload_rows(h, h->z, zh.data()));
        RBL_TRY(upload_rows(h, h->lam, lh.data()));
    }
    labels_changed(h->der);
    if (!h->cfg.objective_only) h->fused_ok = single_sweep_allowed(h);   // (not with labels of its own)
    drop_look_ahead(h->der);
    return RBL_OK;
}

// Row weights of an erm problem: F(w) = (1/n) sum_i c_i loss_i(w) + R(w).  Only the z-step (sigma_i = c_i * sigma0) and
// the logged losses see them; D, G, the w-step, the dual update, the residuals and the rho schedule do not.
int rbl_set_row_weights(rbl_solver* h, const double* c) {
    RBL_ENTER(h);   // like rbl_set_state: a w-step enqueued ahead is put back
    if (h->cfg.weight_function != RBL_W_ERM) {
        rbl_set_error("set_row_weights: row weights need weight_function erm - with weights the sigma of a rank depends on the "
                      "cumulative weight in sorted order, so it is not fixed per rank and the PAV z-step does not apply");
        return RBL_ERR_INVALID;
    }
    if (h->nt != h->n) {
        rbl_set_error("set_row_weights: row-sharded handle (n=%lld of %lld) - row weights are single-device problems",
                      (long long)h->n, (long long)h->nt);
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n;
    if (c) {
        bool any = false;
        for (int64_t i = 0; i < n; ++i) {
            if (!std::isfinite(c[i]) || c[i] < 0.0) {
                rbl_set_error("set_row_weights: c[%lld] = %g - weights are finite and >= 0", (long long)i, c[i]);
                return RBL_ERR_INVALID;
            }
            any = any || c[i] > 0.0;
        }
        if (!any) {
            rbl_set_error("set_row_weights: all %lld weights are zero - at least one must be > 0", (long long)n);
            return RBL_ERR_INVALID;
        }
    }
    RBL_HIP(hipStreamSynchronize(h->stream));
    if (!c) {   // back to the unweighted path; the handle's own buffers alone are freed
        if (h->cw) h->mem.release(h->cw);
        if (h->sigw) h->mem.release(h->sigw);
        h->cw = h->sigw = nullptr;
        h->cw_host.clear();
    } else {
        if (!h->cw) RBL_TRY(h->mem.alloc(&h->cw, (size_t)(n > 0 ? n : 1)));
        if (!h->sigw) RBL_TRY(h->mem.alloc(&h->sigw, (size_t)(n > 0 ? n : 1)));
        std::vector<double> sg((size_t)n);
        for (int64_t i = 0; i < n; ++i) sg[(size_t)i] = c[i] * h->sigma0;   // the ONE product: c == 1.0 gives sigma0's bits
        h->cw_host.assign(c, c + n);
        RBL_HIP(hipMemcpy(h->cw, c, sizeof(double) * n, hipMemcpyHostToDevice));
        RBL_HIP(hipMemcpy(h->sigw, sg.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
    // whatever was computed ahead with the old weights is void: the next z-step runs with the new ones
    row_weights_changed(h->der);
    return RBL_OK;
}

int rbl_get_row_weights(rbl_solver* h, double* c, int* is_set) {
    RBL_ENTER_ITER(h);
    if (is_set) *is_set = h->cw ? 1 : 0;
    if (c)
        for (int64_t i = 0; i < h->n; ++i) c[i] = h->cw ? h->cw_host[(size_t)i] : 1.0;
    return RBL_OK;
}

// One-vs-rest decision on the rows of `data`: cls[i] = argmax_j x_i . w_j (ties: the lowest j).  D = -y X, so the
// scores are -y_i (D w_j)_i: the multi-column V product of the groups (sweep_multi.hip), ceil(k / k_per_pass) passes
// over D, each followed by the row-wise comparison against the best score so far.
int rbl_decide_multi(rbl_solver* h, int k, const double* W, int32_t* cls) {
    RBL_ENTER(h);
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready) {
        rbl_set_error("decide_multi: no data");
        return RBL_ERR_STATE;
    }
    if (k < 1 || k > 64 || !W || !cls) {
        rbl_set_error("decide_multi: 1..64 columns (got %d), W and cls not NULL", k);
        return RBL_ERR_INVALID;
    }
    const int64_t n = h->n, ld = h->ld, d = h->d;
    if (n <= 0) return RBL_OK;
    hipStream_t s = h->stream;
    const bool sparse = h->storage == RBL_STORE_CSR;   // spmv.hip's multi-column pass: the scores keep the single-column bits
    const bool multi = sparse || sweep_multi_supported(h->storage, ld);
    const int kpp = sparse ? RBL_MULTI_KMAX : multi ? sweep_multi_k(h->storage, ld) : 1;
    DevArena mem;   // scratch of this call, freed on return (after the stream wait)
    double *dw = nullptr, *dv = nullptr, *best = nullptr;
    int* dcls = nullptr;
    std::vector<double> wp((size_t)ld * k, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < d; ++i) wp[(size_t)j * ld + i] = W[(size_t)j * d + i];
    RBL_TRY(mem.alloc(&dw, wp.size()));
    RBL_TRY(mem.alloc(&dv, (size_t)n * kpp));
    RBL_TRY(mem.alloc(&best, (size_t)n));
    RBL_TRY(mem.alloc(&dcls, (size_t)n));
    RBL_HIP(hipMemcpy(dw, wp.data(), sizeof(double) * wp.size(), hipMemcpyHostToDevice));
    int rc = RBL_OK;
    for (int j0 = 0; j0 < k && rc == RBL_OK; j0 += kpp) {
        const int kk = std::min(kpp, k - j0);
        if (!multi) {   // outside the multi-column kernels' widths: the single-column pass per column
            rc = launch_gemv(h->storage, h->D, n, ld, dw + (size_t)j0 * ld, dv, h->num_cu, s);
        } else {
            const double* w[RBL_MULTI_KMAX];
            double* v[RBL_MULTI_KMAX];
            for (int j = 0; j < kk; ++j) {
                w[j] = dw + (size_t)(j0 + j) * ld;
                v[j] = dv + (size_t)j * n;
            }
            rc = sparse ? launch_csr_gemv_multi((const CsrStore*)h->D, n, kk, w, v, h->num_cu, s)
                        : launch_sweep_v_multi(h->storage, h->D, n, ld, kk, w, nullptr, nullptr, v, nullptr, nullptr, nullptr, h->num_cu, s);
        }
        if (rc == RBL_OK) rc = launch_decide_rows(n, kk, j0, dv, h->ysign, best, dcls, s);
    }
    if (rc == RBL_OK && (hipMemcpyAsync(cls, dcls, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s) != hipSuccess)) rc = RBL_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && rc == RBL_OK) rc = RBL_ERR_HIP;   // before the scratch goes
    if (rc == RBL_ERR_HIP) rbl_set_error("decide_multi: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

int rbl_get_labels(rbl_solver* h, double* y_out) {
    RBL_ENTER(h);
    if (h->rs) {   // labels of its own (rbl_set_labels)
        for (int64_t i = 0; i < h->n; ++i) y_out[i] = (double)h->ys_host[(size_t)i];
        return RBL_OK;
    }
    std::vector<signed char> t((size_t)h->n);
    RBL_HIP(hipMemcpy(t.data(), h->ysign, (size_t)h->n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < h->n; ++i) y_out[i] = (double)t[i];
    return RBL_OK;
}

int rbl_gram_local(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "gram_local");
    if (!h->data_ready || h->cfg.objective_only) {
        rbl_set_error("gram: no data (or objective-only handle)");
        return RBL_ERR_STATE;
    }
    rbl_gram_report rep{};
    if (h->no_gram) {
        // nothing is formed: the report stays route 0, "no Gram matrix"; rbl_gram_finish takes L through the operator
    } else if (h->storage == RBL_STORE_CSR) {   // the route is the rule's (csr_gram_plan.h); the launcher times itself
        RBL_TRY(launch_csr_gram((const CsrStore*)h->D, h->n, h->ld, h->d, h->slab, h->G, h->num_cu, h->stream, 0, 0, &rep));
    } else {
        struct Ev {   // events of this call alone (the handle's belong to the iteration)
            hipEvent_t e = nullptr;
            ~Ev() {
                if (e) (void)hipEventDestroy(e);
            }
        } e0, e1;
        RBL_HIP(hipEventCreate(&e0.e));
        RBL_HIP(hipEventCreate(&e1.e));
        RBL_HIP(hipEventRecord(e0.e, h->stream));
        RBL_TRY(launch_gram(h->storage, h->D, h->n, h->ld, h->d, h->slab, h->G, h->num_cu, h->stream));
        RBL_HIP(hipEventRecord(e1.e, h->stream));
        RBL_HIP(hipStreamSynchronize(h->stream));
        RBL_HIP(hipEventElapsedTime(&rep.ms, e0.e, e1.e));
        rep.route = 1;
        rep.dense_products = csr_gram_dense_products(h->n, h->ld);
    }
    RBL_HIP(hipStreamSynchronize(h->stream));
    *h->gram_rep = rep;
    gram_formed(h->der);
    return RBL_OK;
}

int rbl_gram_info(rbl_solver* h, rbl_gram_report* out) {
    RBL_ENTER_ITER(h);
    if (!out) {
        rbl_set_error("gram_info: out is NULL");
        return RBL_ERR_INVALID;
    }
    *out = *h->gram_rep;
    return RBL_OK;
}

int rbl_csr_gram_route(int64_t n, int64_t ld, int64_t pair_products) { return csr_gram_route(n, ld, pair_products); }

int rbl_gram_finish(rbl_solver* h) {
    RBL_ENTER(h);
    RBL_NOT_BORROWER(h, "gram_finish");
    if (!h->der.gram_local_done) {
        rbl_set_error("gram_finish before gram_local");
        return RBL_ERR_STATE;
    }
    double lam = 0.0;
    if (h->no_gram) {   // lambda_max(D^T D) by the same 100 steps, D^T (D x) in the place of G x
        OpData op;
        RBL_TRY(op_data(h, &op));
        RBL_TRY(launch_op_power_iteration(op, h->ld, h->d, h->ww.yk, h->ww.Gy, h->ww.scal, 100, &lam, h->stream));
    } else {
        RBL_TRY(launch_power_iteration(h->G, h->ld, h->ww.yk, h->ww.Gy, h->ww.scal, 100, &lam, h->stream));
    }
    gram_changed(h->der);   // G is whole only now (a row shard's was summed over the ranks since rbl_gram_local)
    SharedData& r = *h->sd;   // what comes from G alone goes into the shared record: the borrowers read it there
    r.eig_ok = false;
    r.L = 1.02 * lam;
    if (!(r.L > 0.0)) r.L = 1.0;
    // l2 w-step: RBL_RIDGE_EIG=1 replaces the warm-started CG by a one-time eigendecomposition of G (eig.hip).
    // Opt-in: it makes an iteration 0.13 ms shorter at d = 1000 (14 CG iterations -> 5 small launches when measured, 8 now) but the
    // Jacobi sweeps cost 0.8 s of setup there - 6000 iterations to break even, and a solve runs a few hundred
    static const bool ridge_eig = [] {
        const char* e = getenv("RBL_RIDGE_EIG");
        return e && e[0] == '1';
    }();
    if (h->cfg.wstep == RBL_WSTEP_L2 && h->ld <= 2048 && ridge_eig && !h->no_gram) {
        const size_t nn = (size_t)h->ld * (size_t)h->ld;
        if (!r.eig_Vt) {
            double *Vt = nullptr, *V = nullptr, *lambda = nullptr;
            RBL_TRY(h->shared->alloc(&Vt, nn));   // derived from G alone: shared with the borrowers
            RBL_TRY(h->shared->alloc(&V, nn));
            RBL_TRY(h->shared->alloc(&lambda, (size_t)h->ld));
            r.eig_V = V;
            r.eig_lambda = lambda;
            r.eig_Vt = Vt;   // set last: it says the basis buffers are there
        }
        int rc = RBL_OK, sweeps = 0;
        {
            DevArena tmp;   // Jacobi scratch, freed after the stream wait
            double* Bt = nullptr;
            unsigned long long* off = nullptr;
            RBL_TRY(tmp.alloc(&Bt, nn));
            RBL_TRY(tmp.alloc(&off, 1));
            rc = launch_eig_jacobi(h->G, h->ld, h->d, Bt, r.eig_Vt, r.eig_V, r.eig_lambda, off, h->stream, &sweeps);
            (void)hipStreamSynchronize(h->stream);
        }
        RBL_TRY(rc);
        r.eig_ok = sweeps > 0;
        r.eig_sweeps = sweeps;
    }
    take_gram(h);
    return RBL_OK;
}

int rbl_get_D(rbl_solver* h, double* out) {
    RBL_ENTER(h);
    RBL_TRY(sync_data_epoch(h));
    if (!h->data_ready) {
        rbl_set_error("get_D: no data");
        return RBL_ERR_STATE;
    }
    const int64_t n = h->n, d = h->d;
    int64_t chunk = (64LL << 20) / (8 * d);
    if (chunk < 1) chunk = 1;
    DevArena mem;   // the conversion buffer, freed on return
    double* tmp = nullptr;
    RBL_TRY(mem.alloc(&tmp, (size_t)chunk * d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
        if (h->storage == RBL_STORE_CSR)   // implicit entries: +0.0
            RBL_TRY(launch_csr_dense((const CsrStore*)h->D, r0, rows, d, tmp, h->num_cu, h->stream));
        else
            RBL_TRY(launch_D_to_f64(h->storage, (const char*)h->D + (size_t)r0 * h->ld * h->esz, h->ld, rows, d, tmp, h->stream));
        if (hipMemcpyAsync(out + r0 * d, tmp, sizeof(double) * rows * d, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return RBL_ERR_HIP;
    }
    if (h->rs)   // -y_k * X = r * (-y_owner * X)
        for (int64_t i = 0; i < n; ++i)
            if (h->rs_host[(size_t)i] < 0)
                for (int64_t j = 0; j < d; ++j) out[i * d + j] = -out[i * d + j];
    return RBL_OK;
}

}  // extern "C"
