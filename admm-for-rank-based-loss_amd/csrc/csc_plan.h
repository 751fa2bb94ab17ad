// csc_plan.h - the host arithmetic of the column form of RBL_STORE_CSR (q = D^T c, spmv.hip): every column's entry list
// is cut into segments of at most T entries; segment s of the whole matrix belongs to the column j with
// segptr[j] <= s < segptr[j + 1] and covers the entries [colptr[j] + (s - segptr[j]) T, ... + T) of that column, cut at the
// column's end.  The table is segptr alone: ld + 1 numbers, a function of colptr and T.  No HIP calls: the header is
// compiled by the host compiler alone as well (tests/csc_plan_main.cpp runs it under the sanitizers); under hipcc the
// segment lookup is a device function too, so the kernel and the test run the same arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CSC_PLAN_HD __host__ __device__
#else
#define CSC_PLAN_HD
#endif

// entries of one segment: a power of two in [64, 2048] ("Sparse storage": the measurement that chose it)
#ifndef RBL_CSC_SEG
#define RBL_CSC_SEG 2048
#endif
constexpr int CSC_SEG = RBL_CSC_SEG;
static_assert(CSC_SEG >= 64 && CSC_SEG <= 2048 && (CSC_SEG & (CSC_SEG - 1)) == 0, "segment length: a power of two in [64, 2048]");

// segments of a column of len entries (an empty column has none)
inline int64_t csc_seg_count(int64_t len, int64_t T) { return len > 0 ? (len + T - 1) / T : 0; }

// segptr[0 .. ncols]: first segment of every column; returns the number of segments.  colptr: ncols + 1 entries,
// non-decreasing.
inline int64_t csc_plan_segptr(const int64_t* colptr, int64_t ncols, int64_t T, int64_t* segptr) {
    int64_t s = 0;
    for (int64_t j = 0; j < ncols; ++j) {
        segptr[j] = s;
        s += csc_seg_count(colptr[j + 1] - colptr[j], T);
    }
    segptr[ncols] = s;
    return s;
}

struct CscSegment {
    int64_t col, begin, end;   // entries [begin, end) of the column form, all in column col
};

// segment s of column col (segptr[col] <= s < segptr[col + 1])
CSC_PLAN_HD inline CscSegment csc_segment_at(const int64_t* colptr, const int64_t* segptr, int64_t col, int64_t s, int64_t T) {
    CscSegment g;
    g.col = col;
    g.begin = colptr[col] + (s - segptr[col]) * T;
    g.end = g.begin + T < colptr[col + 1] ? g.begin + T : colptr[col + 1];
    return g;
}

// the column of segment s (0 <= s < segptr[ncols]): the last column j with segptr[j] <= s (columns without segments
// share their successor's segptr and are skipped by "last")
CSC_PLAN_HD inline int64_t csc_segment_col(const int64_t* segptr, int64_t ncols, int64_t s) {
    int64_t lo = 0, hi = ncols;   // invariant: segptr[lo] <= s < segptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (segptr[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

CSC_PLAN_HD inline CscSegment csc_segment(const int64_t* colptr, const int64_t* segptr, int64_t ncols, int64_t s,
                                          int64_t T) {
    return csc_segment_at(colptr, segptr, csc_segment_col(segptr, ncols, s), s, T);
}
