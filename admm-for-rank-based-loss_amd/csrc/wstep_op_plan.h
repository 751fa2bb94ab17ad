// wstep_op_plan.h - how the d-space kernels of the operator w-step (wstep_op.hip) cut a vector of ld doubles, and the
// order in which their sums are taken.  Plain C++ (no HIP): the kernels index through these functions, and
// tests/wstep_op_plan_main.cpp replays them on the host under the sanitizers.
//
// A vector is cut into chunks of OP_CHUNK elements (the last one may be short).  One block of OP_THREADS threads works on a
// chunk at a time: thread t takes the 16-byte packets (two doubles) at chunk offset 2 t + k * 2 OP_THREADS, k = 0 ..
// OP_PACKETS - 1, adds what it finds in that order, and the block folds its threads with block_sum (device_math.h: a
// butterfly inside each wave, then the waves in order).  That is the chunk's partial.  The partials are added in chunk
// order.  Nothing of this depends on the grid: a block walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ..., and a
// chunk's partial is the same whichever block formed it.
#pragma once
#include <cstdint>

constexpr int OP_THREADS = 256;
constexpr int OP_PACKETS = 4;                                 // 16-byte packets per thread and chunk
constexpr int OP_CHUNK = 2 * OP_THREADS * OP_PACKETS;         // 2048 doubles
constexpr int OP_MAX_GRID = 2048;                             // blocks of a launch at most (the rest is walked)

#if defined(__HIPCC__)
#define OP_HD __host__ __device__
#else
#define OP_HD
#endif

// ld is a multiple of 2 (rbl_storage_ld: of 4), so a packet is inside the vector or outside it as a whole
OP_HD inline long long op_num_chunks(long long ld) { return (ld + OP_CHUNK - 1) / OP_CHUNK; }
// first element of packet k of thread t in chunk c; the packet exists when the value is < ld
OP_HD inline long long op_packet(long long c, int t, int k) { return c * OP_CHUNK + (long long)k * 2 * OP_THREADS + 2 * t; }
OP_HD inline int op_grid(long long nchunks) { return (int)(nchunks < 1 ? 1 : nchunks > OP_MAX_GRID ? OP_MAX_GRID : nchunks); }

#if !defined(__HIPCC__)
// The sum of x[0 .. ld) in exactly the order the kernels take it (host replay; ld even)
inline double op_replay_sum(const double* x, long long ld) {
    double total = 0.0;
    for (long long c = 0; c < op_num_chunks(ld); ++c) {
        double v[OP_THREADS];
        for (int t = 0; t < OP_THREADS; ++t) {
            double acc = 0.0;
            for (int k = 0; k < OP_PACKETS; ++k) {
                const long long j = op_packet(c, t, k);
                if (j < ld) {
                    acc += x[j];
                    acc += x[j + 1];
                }
            }
            v[t] = acc;
        }
        double part = 0.0;
        for (int w = 0; w < OP_THREADS / 64; ++w) {   // block_sum: xor butterfly 32, 16, ... 1 inside a wave, waves in order
            double* l = v + 64 * w;
            for (int off = 32; off > 0; off >>= 1) {
                double n[64];
                for (int i = 0; i < 64; ++i) n[i] = l[i] + l[i ^ off];
                for (int i = 0; i < 64; ++i) l[i] = n[i];
            }
            part += l[0];
        }
        total += part;
    }
    return total;
}
#endif
