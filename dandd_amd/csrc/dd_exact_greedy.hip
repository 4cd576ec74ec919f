// dd_exact_greedy.hip -- the walk of dd_exact_greedy over the mask streams of dd_exact_sched.hip (kSchedStream).
//
// A greedy step needs |C U c| of the set C chosen so far and every candidate c, at every k of the window, before it can
// pick.  With the membership masks of every distinct k-mer of every k kept in HBM (8 bytes each, one stream per k, in no
// particular order inside a stream),
//     |C U c|_k = |C|_k + #{ masks m of stream k : m & C == 0 and bit c of m }
// so one launch per step reads every stream once and counts, per k and per bit, the masks that are still LIVE (no bit of
// C) and hold the bit: the GAINS.  The pick itself is host arithmetic on K x 64 numbers (dd_exact_api.hip).
//
//   gains_kernel   A workgroup owns one contiguous range of the concatenated streams; where the range crosses from one
//                  k's stream into the next it flushes and starts over.  A wave takes 64 masks per load (kUnroll loads in
//                  flight), clears the dead ones, and transposes what is left the way the pairwise accumulator of
//                  dd_exact_sched.hip does: one __ballot per bit, a fixed number of trips.  The popcount of a ballot is
//                  the same in every lane, so a wave's counters are scalar registers and a bit costs the vector unit its
//                  test alone.  32 such counters fit beside the loop's own registers, 64 do not (the compiler moves them
//                  in and out of lanes, at three times the vector work), so a wave counts one 32-bit HALF of the masks:
//                  with n <= 32 the four waves take four stripes of 64 masks, above that two waves take the low halves
//                  of two stripes and two the high halves of the same stripes (the second load of a stripe is a cache
//                  hit).  A wave that finds no live mask skips the bits.  Flush, once per workgroup and k: lane b takes
//                  counter b, the waves add up in LDS, 64 threads add to gain[k][b] in HBM.
#include <algorithm>

#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                        // loads of 64 masks a wave has in flight
constexpr unsigned long long kMinRange = 2048;    // masks per workgroup at least: a launch over a few thousand masks is a few workgroups
constexpr unsigned kMaxGrid = 256 * 8;            // 8 workgroups of 4 waves per CU: the registers and the LDS allow all 32 waves

// HALVES = 1 (n <= 32: the upper half of every mask is empty) or 2
template <int HALVES>
__global__ __launch_bounds__(kThreads) void gains_kernel(const uint64_t* __restrict__ store, GreedySegments seg, uint64_t chosen,
                                                       unsigned long long per, unsigned long long* __restrict__ gain) {
    constexpr int kStripes = kThreads / 64 / HALVES;        // stripes of 64 masks the waves of a workgroup take side by side
    constexpr int kTile = kStripes * 64 * kUnroll;          // masks a workgroup takes per trip
    __shared__ unsigned long long wg[64];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t half = wave % HALVES, stripe = wave / HALVES;
    const unsigned long long lo = (unsigned long long)blockIdx.x * per, hi = std::min(lo + per, seg.off[seg.K]);
    for (int kk = 0; kk < seg.K; ++kk) {
        const unsigned long long a = std::max(lo, seg.off[kk]), b = std::min(hi, seg.off[kk + 1]);
        if (a >= b) continue;   // (the same in every thread of the workgroup)
        if (threadIdx.x < 64) wg[threadIdx.x] = 0;
        uint32_t cnt[32];       // wave-uniform: live masks with bit 32 * half + j; a wave sees fewer than 2^32 masks of one stream
#pragma unroll
        for (int j = 0; j < 32; ++j) cnt[j] = 0;
        for (unsigned long long i = a + stripe * 64; i < b; i += kTile) {
            uint64_t m[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const unsigned long long at = i + (unsigned long long)u * (kStripes * 64) + lane;
                m[u] = at < b ? store[at] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const uint64_t live = (m[u] & chosen) ? 0ull : m[u];   // (a mask is never 0: a slot past the range counts nothing either)
                const uint32_t mine = half ? (uint32_t)(live >> 32) : (uint32_t)live;
                if (!__ballot(mine != 0)) continue;
#pragma unroll
                for (int j = 0; j < 32; ++j) cnt[j] += (uint32_t)__builtin_popcountll(__ballot((mine >> j) & 1u));
            }
        }
        uint32_t held = 0;
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if ((int)lane == j) held = cnt[j];
        __syncthreads();
        if (lane < 32 && held) atomicAdd(&wg[32 * half + lane], (unsigned long long)held);
        __syncthreads();
        if (threadIdx.x < 64 && wg[threadIdx.x]) atomicAdd(&gain[(size_t)kk * 64 + threadIdx.x], wg[threadIdx.x]);
        __syncthreads();   // (the next stream of this range zeroes wg)
    }
}

}  // namespace

void launch_exact_greedy_gains(const uint64_t* store, const GreedySegments& seg, int n, uint64_t chosen, unsigned long long* gain_dev,
                               hipStream_t st) {
    const unsigned long long total = seg.off[seg.K];
    if (!total) return;
    unsigned long long per = std::max(kMinRange, (total + kMaxGrid - 1) / kMaxGrid);
    per = (per + 63) / 64 * 64;
    const unsigned grid = (unsigned)((total + per - 1) / per);
    if (n <= 32) hipLaunchKernelGGL(gains_kernel<1>, dim3(grid), dim3(kThreads), 0, st, store, seg, chosen, per, gain_dev);
    else hipLaunchKernelGGL(gains_kernel<2>, dim3(grid), dim3(kThreads), 0, st, store, seg, chosen, per, gain_dev);
}

}  // namespace dd
