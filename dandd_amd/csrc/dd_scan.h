// dd_scan.h -- inclusive prefix sums over a wave and over a workgroup (device only).
// Sums only: the segmented OR-scan of dd_exact_sched.hip has another operator and stays where it is.
#pragma once
#include "dd_common.h"

namespace dd {

// Inclusive sum over the lanes of a wave: lane l gets v(0) + ... + v(l).  T: int, uint32_t, long long, uint64_t.
// WIDTH < 64 (a power of two) runs fewer steps: the caller reads lanes 0 .. WIDTH-1 only (a higher lane sums its last WIDTH).
template <typename T, int WIDTH = 64>
DD_D T wave_incl_sum(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < WIDTH; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// Inclusive sum over a workgroup of NWAVES full waves: returns the calling thread's sum, `total` = the workgroup's.
// Barriers: EVERY thread of the workgroup must call it (uniform control flow).  wave_totals[NWAVES] is LDS of the
// caller's; it is written without a barrier in front -- whoever read it last must have passed one -- and the call ENDS
// with a barrier: when it returns, every thread has read the array and the caller may reuse it at once.
template <int NWAVES, typename T>
DD_D T block_incl_sum(T v, T* wave_totals, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_incl_sum(v);
    if (lane == 63) wave_totals[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (int w = 0; w < NWAVES; ++w) {
        if (w < wave) before += wave_totals[w];
        all += wave_totals[w];
    }
    total = all;
    __syncthreads();
    return before + incl;
}

}  // namespace dd
