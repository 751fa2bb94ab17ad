// csr_plan.h - the host arithmetic of a CSR source (rbl_set_data_csr): the structure checks on indptr, the rows of a
// chunk, the entries a chunk covers and the offset its indptr slice is rebased by.  No HIP calls: the header is compiled
// by the host compiler alone as well (tests/csr_plan_main.cpp runs it under the sanitizers).
#pragma once
#include <cstdint>

enum { CSR_PLAN_OK = 0, CSR_PLAN_FIRST = 1, CSR_PLAN_DECREASING = 2, CSR_PLAN_LAST = 3 };

// indptr (n + 1 entries of type I) is a row partition of nnz entries: indptr[0] == 0, non-decreasing, indptr[n] == nnz.
// Every entry then lies in [0, nnz].  *row: the row whose end lies before its start (CSR_PLAN_DECREASING); *got: the
// offending value.
template <typename I>
inline int csr_check_indptr(const I* indptr, int64_t n, int64_t nnz, int64_t* row, int64_t* got) {
    *row = 0;
    *got = (int64_t)indptr[0];
    if ((int64_t)indptr[0] != 0) return CSR_PLAN_FIRST;
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) {
            *row = r;
            *got = (int64_t)indptr[r + 1];
            return CSR_PLAN_DECREASING;
        }
    *got = (int64_t)indptr[n];
    if ((int64_t)indptr[n] != nnz) return CSR_PLAN_LAST;
    return CSR_PLAN_OK;
}

// the 64-bit copy every later step plans on (int32 and int64 sources alike)
template <typename I>
inline void csr_widen_indptr(const I* indptr, int64_t n, int64_t* out) {
    for (int64_t r = 0; r <= n; ++r) out[r] = (int64_t)indptr[r];
}

// rows of one chunk: as many dense staging rows of row_bytes as fit chunk_bytes, at least one, at most n; with
// block > 0 a whole number of row blocks (the statistics of RBL_SCALE_FIT run over blocks of 1024 rows), at least one
inline int64_t csr_chunk_rows(int64_t chunk_bytes, int64_t row_bytes, int64_t n, int64_t block) {
    int64_t rows = row_bytes > 0 ? chunk_bytes / row_bytes : n;
    if (block > 0) {
        rows = rows / block * block;
        if (rows < block) rows = block;
    }
    if (rows < 1) rows = 1;
    if (rows > n) rows = n;
    return rows;
}

inline int64_t csr_chunk_count(int64_t n, int64_t chunk) { return chunk > 0 ? (n + chunk - 1) / chunk : 0; }

// chunk k: rows [r0, r0 + rows), entries [base, base + cnt) of indices / values.  The chunk's indptr slice is
// indptr[r0 .. r0 + rows] (rows + 1 entries); entry positions inside the chunk's own slices of indices / values are
// indptr[r] - base.  An empty chunk (rows of no entries) has cnt == 0.
struct CsrChunk {
    int64_t r0, rows, base, cnt;
};
inline CsrChunk csr_chunk(const int64_t* ip, int64_t n, int64_t chunk, int64_t k) {
    CsrChunk c;
    c.r0 = k * chunk;
    c.rows = n - c.r0 < chunk ? n - c.r0 : chunk;
    c.base = ip[c.r0];
    c.cnt = ip[c.r0 + c.rows] - c.base;
    return c;
}

// the entries of the fullest chunk: what the two staging slices of a host source are sized to
inline int64_t csr_max_chunk_nnz(const int64_t* ip, int64_t n, int64_t chunk) {
    int64_t m = 0;
    for (int64_t k = 0; k < csr_chunk_count(n, chunk); ++k) {
        const int64_t c = csr_chunk(ip, n, chunk, k).cnt;
        if (c > m) m = c;
    }
    return m;
}
