// Stand-alone check of csrc/wstep_op_plan.h (how the d-space kernels of the operator w-step cut a vector into chunks and
// in which order they add): compiled by the host compiler with -fsanitize=address,undefined and run by
// tests/test_wstep_op_host.py.  Every packet is looked up the way the kernels look it up, in a vector of exactly ld
// doubles, for every grid a launch may have: a plan that is off by one is an out-of-bounds access or a miscount here.
#include "../admm-for-rank-based-loss_amd/csrc/wstep_op_plan.h"

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

// the kernels' walk with `grid` blocks: every element of [0, ld) is touched exactly once, none beyond; one partial per chunk
static void replay(long long ld, int grid) {
    std::vector<int> hits((size_t)ld, 0);
    const long long nc = op_num_chunks(ld);
    std::vector<int> part((size_t)nc, 0);
    CHECK(nc * OP_CHUNK >= ld && (nc - 1) * OP_CHUNK < ld);
    for (int b = 0; b < grid; ++b)
        for (long long c = b; c < nc; c += grid) {
            part[(size_t)c] += 1;
            for (int t = 0; t < OP_THREADS; ++t)
                for (int k = 0; k < OP_PACKETS; ++k) {
                    const long long j = op_packet(c, t, k);
                    CHECK(j >= c * OP_CHUNK && j + 1 < (c + 1) * OP_CHUNK);
                    if (j < ld) {
                        CHECK(j + 1 < ld);   // a packet is inside as a whole (ld even)
                        hits[(size_t)j] += 1;
                        hits[(size_t)j + 1] += 1;
                    }
                }
        }
    for (long long j = 0; j < ld; ++j) CHECK(hits[(size_t)j] == 1);
    for (long long c = 0; c < nc; ++c) CHECK(part[(size_t)c] == 1);
}

int main() {
    CHECK(OP_CHUNK == 2 * OP_THREADS * OP_PACKETS && OP_THREADS % 64 == 0);
    const long long C = OP_CHUNK;
    for (long long ld : {4LL, 40LL, C - 4, C, C + 4, 2 * C, 2 * C + 4, 16384LL, 16388LL, 20000LL, 200000LL, 1000000LL}) {
        CHECK(op_grid(op_num_chunks(ld)) >= 1 && op_grid(op_num_chunks(ld)) <= OP_MAX_GRID);
        for (int grid : {1, 2, 7, op_grid(op_num_chunks(ld)), OP_MAX_GRID}) replay(ld, grid);
    }
    // the sum's order: integers add exactly in any order; a vector whose sum depends on the order gives the same bits for
    // every call (the order is a function of ld alone)
    for (long long ld : {40LL, C, C + 4, 2 * C + 4, 20000LL}) {
        std::vector<double> x((size_t)ld);
        for (long long j = 0; j < ld; ++j) x[(size_t)j] = (double)(j % 17) - 8.0;
        double want = 0.0;
        for (long long j = 0; j < ld; ++j) want += x[(size_t)j];
        CHECK(op_replay_sum(x.data(), ld) == want);
        for (long long j = 0; j < ld; ++j) x[(size_t)j] = 1.0 / (double)(j + 3);
        const double a = op_replay_sum(x.data(), ld), b = op_replay_sum(x.data(), ld);
        CHECK(a == b && a > 0.0);
    }
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("wstep_op_plan: ok\n");
    return 0;
}
