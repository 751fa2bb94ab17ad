// Stand-alone check of csrc/csc_plan.h (the segment plan of q = D^T c on sparse storage): compiled by the host compiler with
// -fsanitize=address,undefined and run by tests/test_csr_storage_host.py.  Every segment is looked up the way the kernel
// looks it up, in tables of exactly the planned sizes, and marks its entries in a buffer of exactly nnz slots, so that a
// plan that is off by one is an out-of-bounds access or a miscount here.
#include "../admm-for-rank-based-loss_amd/csrc/csc_plan.h"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                              \
        }                                                         \
    } while (0)

// columns of the given lengths, segments of at most T entries
static void replay(const std::vector<int64_t>& len, int64_t T) {
    const int64_t ncols = (int64_t)len.size();
    std::vector<int64_t> colptr((size_t)ncols + 1), segptr((size_t)ncols + 1);
    colptr[0] = 0;
    for (int64_t j = 0; j < ncols; ++j) colptr[(size_t)j + 1] = colptr[(size_t)j] + len[(size_t)j];
    const int64_t nnz = colptr[(size_t)ncols];
    const int64_t nseg = csc_plan_segptr(colptr.data(), ncols, T, segptr.data());
    CHECK(segptr[0] == 0 && segptr[(size_t)ncols] == nseg);
    int64_t expect = 0;
    for (int64_t j = 0; j < ncols; ++j) {
        CHECK(segptr[(size_t)j] == expect);
        CHECK(csc_seg_count(len[(size_t)j], T) == (len[(size_t)j] + T - 1) / T);
        expect += csc_seg_count(len[(size_t)j], T);
    }
    CHECK(expect == nseg);
    std::vector<int> owner((size_t)nnz, 0);       // segments that cover the entry
    std::vector<double> part((size_t)nseg, 0.0);  // the partial sums' buffer: one slot per segment
    int64_t prev_col = -1, prev_end = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const CscSegment g = csc_segment(colptr.data(), segptr.data(), ncols, s, T);
        CHECK(g.col >= 0 && g.col < ncols);
        if (g.col < 0 || g.col >= ncols) continue;
        // inside its column, not empty, at most T entries
        CHECK(g.begin >= colptr[(size_t)g.col] && g.end <= colptr[(size_t)g.col + 1]);
        CHECK(g.end > g.begin && g.end - g.begin <= T);
        // the segments of a column are consecutive and in order: the first starts the column, every other one starts where
        // the one before ended, and all but the last are full
        CHECK(g.col >= prev_col);
        if (g.col != prev_col) {
            CHECK(g.begin == colptr[(size_t)g.col] && s == segptr[(size_t)g.col]);
            if (prev_col >= 0) CHECK(prev_end == colptr[(size_t)prev_col + 1]);
            for (int64_t j = prev_col + 1; j < g.col; ++j) CHECK(len[(size_t)j] == 0);   // only empty columns are skipped
        } else {
            CHECK(g.begin == prev_end && g.begin - colptr[(size_t)g.col] == (s - segptr[(size_t)g.col]) * T);
        }
        if (g.end < colptr[(size_t)g.col + 1]) CHECK(g.end - g.begin == T);
        for (int64_t k = g.begin; k < g.end; ++k) owner[(size_t)k] += 1;
        part[(size_t)s] = (double)(g.end - g.begin);
        prev_col = g.col;
        prev_end = g.end;
    }
    if (prev_col >= 0) CHECK(prev_end == colptr[(size_t)prev_col + 1]);
    for (int64_t j = prev_col + 1; j < ncols; ++j) CHECK(len[(size_t)j] == 0);
    for (int64_t k = 0; k < nnz; ++k) CHECK(owner[(size_t)k] == 1);   // every entry belongs to exactly one segment
    // the second kernel: a column's partial sums are the slots segptr[j] .. segptr[j + 1]
    for (int64_t j = 0; j < ncols; ++j) {
        double sum = 0.0;
        for (int64_t s = segptr[(size_t)j]; s < segptr[(size_t)j + 1]; ++s) sum += part[(size_t)s];
        CHECK(sum == (double)len[(size_t)j]);
    }
}

int main() {
    CHECK(CSC_SEG >= 64 && CSC_SEG <= 2048 && (CSC_SEG & (CSC_SEG - 1)) == 0);
    for (int T32 : {64, 128, 256, 512, 1024, 2048, (int)CSC_SEG}) {
        const int64_t T = T32;
        replay({}, T);   // no columns
        for (int64_t one : {(int64_t)0, (int64_t)1, T - 1, T, T + 1, 2 * T + 1}) replay({one}, T);
        replay({0, 1, T - 1, T, T + 1, 2 * T + 1}, T);
        replay({2 * T + 1, T + 1, T, T - 1, 1, 0}, T);
        replay({0, 0, 0, 5, 0, 0, T, 0, 0, 3 * T, 0, 0, 0}, T);   // runs of empty columns: first, in the middle, last
        replay({0, 0, 0, 0}, T);                                  // no entries at all
        replay({0, 0, 7 * T + 5, 0, 0}, T);                       // one column holds every entry
        replay({100000}, T);
        std::vector<int64_t> many;
        for (int j = 0; j < 3000; ++j) many.push_back((int64_t)((j * 2654435761u) % (unsigned)(3 * T)) * (j % 7 != 0));
        replay(many, T);
    }
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("csc_plan: ok\n");
    return 0;
}
