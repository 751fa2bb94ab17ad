// Stand-alone check of csrc/csr_plan.h (the host arithmetic of a CSR source): compiled by the host compiler with
// -fsanitize=address,undefined and run by tests/test_csr_host.py.  Every chunk's slices are walked the way the upload
// walks them, in buffers of exactly the planned sizes, so that a plan that is off by one is an out-of-bounds access here.
#include "../admm-for-rank-based-loss_amd/csrc/csr_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                              \
        }                                                         \
    } while (0)

static uint64_t lcg_state = 12345;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

// A matrix of n rows whose row r holds len[r] entries: builds indptr in type I, checks it, widens it, cuts it into
// chunks and replays every chunk with freshly allocated slices of the planned sizes.
template <typename I>
static void replay(const std::vector<int64_t>& len, int64_t chunk_bytes, int64_t row_bytes, int64_t block) {
    const int64_t n = (int64_t)len.size();
    std::vector<I> indptr((size_t)n + 1);
    indptr[0] = 0;
    for (int64_t r = 0; r < n; ++r) indptr[(size_t)r + 1] = (I)(indptr[(size_t)r] + (I)len[(size_t)r]);
    const int64_t nnz = (int64_t)indptr[(size_t)n];
    std::vector<int64_t> entry((size_t)nnz);   // the "indices / values" of the source: entry k holds k
    for (int64_t k = 0; k < nnz; ++k) entry[(size_t)k] = k;

    int64_t row = -1, got = -1;
    CHECK(csr_check_indptr(indptr.data(), n, nnz, &row, &got) == CSR_PLAN_OK);
    std::vector<int64_t> ip((size_t)n + 1);
    csr_widen_indptr(indptr.data(), n, ip.data());
    for (int64_t r = 0; r <= n; ++r) CHECK(ip[(size_t)r] == (int64_t)indptr[(size_t)r]);
    if (n == 0) {
        CHECK(csr_chunk_count(n, 1) == 0);
        return;
    }

    const int64_t chunk = csr_chunk_rows(chunk_bytes, row_bytes, n, block);
    CHECK(chunk >= 1 && chunk <= n);
    if (block > 0 && chunk < n) CHECK(chunk % block == 0);
    if (block == 0 && row_bytes > 0 && chunk > 1) CHECK(chunk * row_bytes <= chunk_bytes);
    const int64_t nk = csr_chunk_count(n, chunk);
    const int64_t cap = csr_max_chunk_nnz(ip.data(), n, chunk);
    int64_t rows_seen = 0, entries_seen = 0, fullest = 0;
    for (int64_t k = 0; k < nk; ++k) {
        const CsrChunk c = csr_chunk(ip.data(), n, chunk, k);
        CHECK(c.r0 == rows_seen && c.rows >= 1 && c.r0 + c.rows <= n);
        CHECK(c.base == entries_seen && c.cnt >= 0 && c.cnt <= cap);
        // the three copies of the upload, into buffers of the planned sizes
        std::vector<I> ip_slice((size_t)c.rows + 1);
        std::memcpy(ip_slice.data(), indptr.data() + c.r0, sizeof(I) * (size_t)(c.rows + 1));
        std::vector<int64_t> slice((size_t)cap);
        if (c.cnt > 0) std::memcpy(slice.data(), entry.data() + c.base, sizeof(int64_t) * (size_t)c.cnt);
        // what the expand kernel does with them: rebased entry positions of every row
        for (int64_t r = 0; r < c.rows; ++r) {
            const int64_t a = (int64_t)ip_slice[(size_t)r] - c.base, b = (int64_t)ip_slice[(size_t)r + 1] - c.base;
            CHECK(a >= 0 && a <= b && b <= c.cnt);
            CHECK(b - a == len[(size_t)(c.r0 + r)]);
            for (int64_t p = a; p < b; ++p) CHECK(slice[(size_t)p] == c.base + p);
        }
        rows_seen += c.rows;
        entries_seen += c.cnt;
        if (c.cnt > fullest) fullest = c.cnt;
    }
    CHECK(rows_seen == n && entries_seen == nnz && fullest == cap);
}

template <typename I>
static void structure_checks() {
    int64_t row = -1, got = -1;
    {
        const I ok[4] = {0, 2, 2, 5};
        CHECK(csr_check_indptr(ok, 3, 5, &row, &got) == CSR_PLAN_OK);
        CHECK(csr_check_indptr(ok, 3, 4, &row, &got) == CSR_PLAN_LAST && got == 5);
        CHECK(csr_check_indptr(ok, 3, 6, &row, &got) == CSR_PLAN_LAST && got == 5);
    }
    {
        const I first[3] = {1, 2, 3};
        CHECK(csr_check_indptr(first, 2, 3, &row, &got) == CSR_PLAN_FIRST && got == 1);
    }
    {
        const I dec[5] = {0, 3, 2, 4, 4};
        CHECK(csr_check_indptr(dec, 4, 4, &row, &got) == CSR_PLAN_DECREASING && row == 1 && got == 2);
    }
    {
        const I neg[3] = {0, (I)-1, 0};
        CHECK(csr_check_indptr(neg, 2, 0, &row, &got) == CSR_PLAN_DECREASING && row == 0 && got == -1);
    }
    {
        const I empty[1] = {0};   // no rows
        CHECK(csr_check_indptr(empty, 0, 0, &row, &got) == CSR_PLAN_OK);
        CHECK(csr_check_indptr(empty, 0, 1, &row, &got) == CSR_PLAN_LAST);
    }
}

int main() {
    structure_checks<int32_t>();
    structure_checks<int64_t>();
    {   // int64 values an int32 cannot hold
        const int64_t big[3] = {0, (int64_t)1 << 33, (int64_t)1 << 34};
        int64_t row = -1, got = -1;
        CHECK(csr_check_indptr(big, 2, (int64_t)1 << 34, &row, &got) == CSR_PLAN_OK);
        std::vector<int64_t> ip(3);
        csr_widen_indptr(big, 2, ip.data());
        const CsrChunk c = csr_chunk(ip.data(), 2, 1, 1);
        CHECK(c.r0 == 1 && c.rows == 1 && c.base == ((int64_t)1 << 33) && c.cnt == ((int64_t)1 << 33));
        CHECK(csr_max_chunk_nnz(ip.data(), 2, 1) == ((int64_t)1 << 33));
    }
    // chunk rows
    CHECK(csr_chunk_rows(64 << 20, 4000, 1000000, 0) == 16777);
    CHECK(csr_chunk_rows(64 << 20, 4000, 1000000, 1024) == 16384);
    CHECK(csr_chunk_rows(100, 4000, 1000000, 1024) == 1024);   // at least one block
    CHECK(csr_chunk_rows(100, 4000, 500, 1024) == 500);        // ... of a short matrix
    CHECK(csr_chunk_rows(100, 4000, 7, 0) == 1);               // at least one row
    CHECK(csr_chunk_rows(1 << 30, 8, 7, 0) == 7);              // at most n

    std::vector<std::vector<int64_t>> shapes;
    shapes.push_back({});                                 // no rows
    shapes.push_back({0});                                // one empty row
    shapes.push_back({5});
    shapes.push_back({0, 0, 0, 0, 0, 0, 0});              // nnz == 0: every chunk is empty
    shapes.push_back({0, 3, 0, 0, 0, 7, 1, 0});           // empty first and last row, a run of empty rows
    {
        std::vector<int64_t> v;
        for (int r = 0; r < 2500; ++r) v.push_back(r % 97 == 0 ? 0 : (int64_t)(lcg() % 40));
        shapes.push_back(v);
        for (int r = 1030; r < 2060; ++r) v[(size_t)r] = 0;   // a whole empty chunk in the middle
        shapes.push_back(v);
    }
    for (const std::vector<int64_t>& len : shapes)
        for (int64_t row_bytes : {8, 400, 4004})
            for (int64_t chunk_bytes : {1, 4004, 50000, 1 << 20, 1 << 30})
                for (int64_t block : {0, 1024}) {
                    replay<int32_t>(len, chunk_bytes, row_bytes, block);
                    replay<int64_t>(len, chunk_bytes, row_bytes, block);
                }
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("csr_plan: ok\n");
    return 0;
}
