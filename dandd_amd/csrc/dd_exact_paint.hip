// dd_exact_paint.hip -- samples that are no leaves, painted window by window with the genomes of an exact universe.
//
// dd_exact_screen.hip answers "how much of sample s does genome i hold" with one number per file; this keeps the position.
// Behind the same ordered records (a LocateSet, launch_exact_emit_order) one kernel walks every sample and leaves, for
// every window of W tokens of its token stream, a row of n + 2 counters: the tokens of the window at which a valid k-mer
// ends, at which that k-mer is a record of the universe, and at which its membership mask has bit i, for every genome i.
// Counts are over positions: a k-mer that stands three times in a window counts three times.
//
//   paint    paint_kernel: one thread per 64-token segment, one launch unit (gridDim.y) per sample -- screen_kernel's
//            shape, walk and lookup (walk_segment and find_record of dd_exact_walk.h).  A hit at record r loads
//            set.mask[r] and adds it to the thread's per-genome counters.
//
// How a thread counts 64 genomes per hit without 64 adds: the counters are a bit-sliced VERTICAL counter, kPaintPlanes
// 64-bit planes; bit i of plane j is bit j of genome i's count.  Adding a mask is a ripple carry over the planes -- an
// `and` and an `xor` per plane, no loop over genomes.  A segment ends at most 64 k-mers, so a count is at most
// 64 = 1000000b: seven planes hold it and nothing is flushed mid-way (the flush every 2^planes records that kept this form
// out of tally_kernel does not arise: a thread's run IS 64 records).  Columns 0 and 1 are two plain integers.
//
// How the planes reach the window's row, by the window's size in segments:
//   one segment (W = 64)      the thread owns its row: plain stores of all n + 2 columns.
//   the wave in one window    the 64 segments of a wave are consecutive; where the first and the last live one lie in the
//                             same window (always so when W is a multiple of 4096), column i of plane j over the wave is one
//                             __ballot, lane i adds its popcount shifted by the plane's weight, and the wave issues one
//                             no-return atomicAdd per non-zero genome: n + 2 atomics per 64 segments at the most.  A plane
//                             that is zero in every lane costs one ballot.
//   otherwise                 (a window border inside the wave) every live thread adds its non-zero counts to its own
//                             window's row.
// Integer sums: the order of arrival does not change them, two calls return identical bytes.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void paint_kernel(const ExactGenome* __restrict__ samples, int k, LocateSet set, int n,
                                                   unsigned long long wsegs, const unsigned long long* __restrict__ row0,
                                                   uint32_t* counts) {
    const ExactGenome* u = samples + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long first = seg - (unsigned)lane;   // the wave's first segment: live if any of them is
    if (first * kSegTokens >= ntok) return;
    const bool live = seg * kSegTokens < ntok;
    PlaneCounter pc;
    pc.clear();
    uint32_t valid = 0, inpan = 0;
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long, int, uint64_t ah, uint64_t al, bool) {
        ++valid;
        unsigned long long r;
        if (find_record<WIDE>(set, ah, al, r)) ++inpan, pc.add(set.mask[r]);
    });
    const unsigned long long ncol = (unsigned long long)n + 2;
    // (the host has checked that the sample owns ceil(ntok / W) rows from row0 on: a live segment's window is one of them)
    uint32_t* rows = counts + row0[blockIdx.y] * ncol;
    if (wsegs == 1) {
        if (!live) return;
        uint32_t* row = rows + seg * ncol;
        row[0] = valid, row[1] = inpan;
        for (int i = 0; i < n; ++i) row[2 + i] = pc.count(i);
        return;
    }
    unsigned long long w;
    if (wave_in_one_window(first, ntok, wsegs, w)) pc.flush_wave(rows + w * ncol, n, lane, valid, inpan);
    else if (live) pc.flush(rows + (seg / wsegs) * ncol, n, valid, inpan);
}

}  // namespace

void launch_exact_paint(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set, int n,
                        size_t window_segments, const unsigned long long* row0_dev, uint32_t* counts_dev, hipStream_t st) {
    if (ns <= 0 || !max_segments) return;
    launch_segment_walk((size_t)ns, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((paint_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, samples_dev, k, set, n,
                           (unsigned long long)window_segments, row0_dev, counts_dev);
    });
}

}  // namespace dd
