// dd_exact_cover.hip -- samples that are no leaves, laid along the GENOMES of an exact universe: per window of a target genome's
// token stream, how many of its k-mer positions a sample holds and how deep.
//
// dd_exact_paint.hip windows the sample; dd_exact_depth.hip leaves one 32-bit counter per (sample, record) and bins it per
// genome.  Here the windows are a universe genome's and the counters are depth_kernel's, used as they are.  What joins them
// is the record a genome position maps to, and that does not depend on the sample: the lookup -- ceil(log2 found) dependent
// loads per position, the expensive part of every kernel of this family -- is paid once per target position, not once per
// (position, sample).  Two kernels:
//
//   index    cover_index_kernel: once per call, over the target genomes only.  locate_kernel's shape: one thread per 64-token
//            segment, one launch unit (gridDim.y) per target, walk_segment and find_record of dd_exact_walk.h.  For every
//            token of its segment the thread stores one 32-bit word: kCoverNone where no valid k-mer ends (the tokens behind
//            ntok are BREAKs: the same), else the record's index, with kCoverPrivate set where the record's mask is exactly
//            1 << g -- the k-mer is private to this genome within the universe.  The thread owns its 64 words: plain stores.
//            The emission is (0, 0), so every valid k-mer of a universe genome IS a record: a miss cannot happen and nothing
//            diagnoses one (a word that were not found would stay kCoverNone: no index leaves the records).
//   cover    cover_kernel: once per round of samples, grid (segments of the target, target, sample of the round).  A thread
//            reads the 64 index words of its segment, gathers count[s][r] for the valid ones and keeps six per-segment counts
//            in registers (dd_kernels.h: valid, covered, depth, private, private_covered, private_depth; a depth is
//            min(c, clip), clip <= 1023: a segment's sum stays below 2^16, a window's of 2^22 positions below 2^32).  A window
//            is whole segments, so a segment lies in one window, and the six counts reach the window's row as paint_kernel's
//            planes do: by plain stores where the window is one segment (the thread owns the row); by a wave reduction and one
//            no-return atomicAdd per non-zero column where the wave's live segments lie in one window (known before the
//            gather; always so when the window is a multiple of 4096 tokens); by per-thread no-return atomics of the non-zero
//            counts at a window border inside the wave.  No global atomic per position.  Integer sums: the order of arrival
//            does not change them, two calls return identical bytes.
//
// How the 64 index words are read: 16 x uint4 per thread, the segment's own 256 bytes.  A lane-per-token layout (a wave
// loads 64 consecutive words with one instruction, 64 segments transposed through LDS so that a thread still sums its own
// segment) would make every load instruction one contiguous KiB, at 16 KiB of LDS per wave or a barrier per 16-token piece.
// The thread-per-segment form touches the same cache lines -- each thread its own two 128-byte lines, every byte of which it
// uses within the next loads -- and the stream it reads is 4 sequential bytes per position against the gather's one random
// 4-byte word per position, which costs a whole line from L2 or beyond and is what the kernel waits for.  The form without
// LDS keeps the occupancy that hides that latency and needs no barrier; four loads are issued ahead of their sixteen gathers.
// This was decided by reading the two kernels, not by a measurement of both forms.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void cover_index_kernel(const CoverUnit* __restrict__ units, int k, LocateSet set,
                                                         uint32_t* __restrict__ index) {
    const CoverUnit* u = units + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (seg * kSegTokens >= ntok) return;
    // (the host has carved ceil(ntok / 64) * 64 words from u->index on: a live segment's words are among them)
    uint32_t* mine = index + u->index + seg * kSegTokens;
    const uint64_t own = 1ull << u->genome;
    int next = 0;   // the first token of the segment without a word yet
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long, int t, uint64_t ah, uint64_t al, bool) {
        unsigned long long r;
        if (!find_record<WIDE>(set, ah, al, r)) return;
        for (; next < t; ++next) mine[next] = kCoverNone;
        mine[t] = (uint32_t)r | (set.mask[r] == own ? kCoverPrivate : 0u);   // (r < found < 2^31: the host has checked)
        next = t + 1;
    });
    for (; next < (int)kSegTokens; ++next) mine[next] = kCoverNone;
}

// the sum over the wave, the same in every lane
DD_D uint32_t cover_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__global__ __launch_bounds__(256) void cover_kernel(const CoverUnit* __restrict__ units, const uint32_t* __restrict__ index,
                                                   const uint32_t* __restrict__ count, unsigned long long found,
                                                   unsigned long long wsegs, uint32_t clip, unsigned long long nrows, uint32_t* rows) {
    const CoverUnit* u = units + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long first = seg - (unsigned)lane;   // the wave's first segment: live if any of them is
    if (first * kSegTokens >= ntok) return;
    const bool live = seg * kSegTokens < ntok;
    const uint32_t* mine = count + (unsigned long long)blockIdx.z * found;
    uint32_t c[kCoverColumns];
#pragma unroll
    for (int j = 0; j < kCoverColumns; ++j) c[j] = 0;
    if (live) {
        const uint4* words = reinterpret_cast<const uint4*>(index + u->index + seg * kSegTokens);   // (256-byte aligned)
#pragma unroll 4
        for (int i = 0; i < (int)kSegTokens / 4; ++i) {
            const uint4 w4 = words[i];
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (w[j] == kCoverNone) continue;
                const uint32_t d = mine[w[j] & ~kCoverPrivate];   // (an index word holds a record: inside the row)
                const uint32_t has = d ? 1u : 0u, dc = d < clip ? d : clip, priv = w[j] >> 31;
                c[0] += 1, c[1] += has, c[2] += dc;
                c[3] += priv, c[4] += priv & has, c[5] += priv ? dc : 0u;
            }
        }
    }
    // (the host has checked that the target owns ceil(ntok / W) rows from u->row0 on: a live segment's window is one of them)
    uint32_t* base = rows + ((unsigned long long)blockIdx.z * nrows + u->row0) * kCoverColumns;
    if (wsegs == 1) {
        if (!live) return;
        uint32_t* row = base + seg * kCoverColumns;
#pragma unroll
        for (int j = 0; j < kCoverColumns; ++j) row[j] = c[j];
        return;
    }
    unsigned long long w;
    if (wave_in_one_window(first, ntok, wsegs, w)) {   // (the same in every lane; the lanes behind the stream hold zeros)
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < kCoverColumns; ++j) {
            const uint32_t s = cover_wave_sum(c[j]);
            if (lane == j) sum = s;
        }
        if (lane < kCoverColumns && sum) atomicAdd(base + w * kCoverColumns + lane, sum);
        return;
    }
    if (!live) return;
    uint32_t* row = base + (seg / wsegs) * kCoverColumns;
#pragma unroll
    for (int j = 0; j < kCoverColumns; ++j)
        if (c[j]) atomicAdd(row + j, c[j]);
}

}  // namespace

void launch_exact_cover_index(const CoverUnit* units_dev, int nunits, size_t max_segments, int k, int canonical, const LocateSet& set,
                              uint32_t* index_dev, hipStream_t st) {
    if (nunits <= 0 || !max_segments || !set.found) return;
    launch_segment_walk((size_t)nunits, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((cover_index_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, units_dev, k, set, index_dev);
    });
}

void launch_exact_cover(const CoverUnit* units_dev, int nunits, size_t max_segments, const uint32_t* index_dev, const uint32_t* count_dev,
                        size_t found, int ns, size_t window_segments, uint32_t clip, size_t nrows, uint32_t* rows_dev, hipStream_t st) {
    if (nunits <= 0 || ns <= 0 || !max_segments || !found) return;
    const dim3 grid((unsigned)((max_segments + 255) / 256), (unsigned)nunits, (unsigned)ns), block(256);
    hipLaunchKernelGGL(cover_kernel, grid, block, 0, st, units_dev, index_dev, count_dev, (unsigned long long)found,
                       (unsigned long long)window_segments, clip, (unsigned long long)nrows, rows_dev);
}

}  // namespace dd
