// dd_exact_runs.h -- the runs of the sorted k-mer array, for the kernels that reduce them to membership (dd_exact_sched.hip:
// a 64-bit mask per distinct k-mer; dd_exact_wide.hip: a row of up to four such words): the view of the sorted array, the
// slots of a thread with their run borders and genomes, the segmented OR-scan of a workgroup, the scan of one chunk over one
// 64-genome window, and the one round of wave aggregation the histograms add through.  Everything here is inlined into its
// caller: no kernel calls across files.
#pragma once
#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kThreads = 256, kItems = 8, kChunk = kThreads * kItems;  // slots per chunk = masks an LDS tile can hold
constexpr int kCarryThreads = 1024;

struct SortedView {
    const uint64_t* lo;
    const uint64_t* hi;
    const uint8_t* g;   // null: the genome is the top byte of the most significant word
    uint64_t mlo, mhi;
    size_t count;
    int n;              // genomes: a tag outside 0..n-1 sets no bit
};

// (flag, value) pairs under  (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 | v2): the segmented OR.  Inclusive scan over
// the workgroup; returns the exclusive prefix of the calling thread in (ef, ev) and the workgroup's total in (tf, tv).
template <int NWAVES>
DD_D void block_seg_scan(uint32_t f, uint64_t v, uint32_t* sf, uint64_t* sv, uint32_t& ef, uint64_t& ev, uint32_t& tf,
                         uint64_t& tv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t of = __shfl_up(f, d);
        const uint64_t ov = __shfl_up((unsigned long long)v, d);
        if (lane >= d) {
            if (!f) v |= ov;
            f |= of;
        }
    }
    if (lane == 63) sf[wave] = f, sv[wave] = v;
    uint32_t xf = __shfl_up(f, 1);
    uint64_t xv = __shfl_up((unsigned long long)v, 1);
    if (lane == 0) xf = 0, xv = 0;
    __syncthreads();
    uint32_t pf = 0;
    uint64_t pv = 0;
    tf = 0, tv = 0;
    for (int q = 0; q < NWAVES; ++q) {
        const uint32_t wf = sf[q];
        const uint64_t wv = sv[q];
        if (q == wave) pf = tf, pv = tv;
        tv = wf ? wv : (tv | wv);
        tf |= wf;
    }
    ef = pf | xf;
    ev = xf ? xv : (pv | xv);
}

// the calling thread's kItems consecutive slots of a chunk: which start a run, which end one, and tag(j, genome) for slot j
// with the genome it carries (0xFF: a slot behind the array, or one nothing wrote)
template <bool WIDE, class F>
DD_D void load_slots(const SortedView& s, size_t first, uint32_t& head, uint32_t& tail, F&& tag) {
    head = tail = 0;
    uint64_t pl = 0, ph = 0;
    bool pvalid = first > 0 && first - 1 < s.count;
    if (pvalid) {
        pl = s.lo[first - 1] & s.mlo;
        if (WIDE) ph = s.hi[first - 1] & s.mhi;
    }
#pragma unroll
    for (int j = 0; j <= kItems; ++j) {
        const size_t i = first + j;
        const bool valid = i < s.count;
        uint64_t rl = 0, rh = 0;
        if (valid) {
            rl = s.lo[i];
            if (WIDE) rh = s.hi[i];
        }
        const uint64_t cl = rl & s.mlo, ch = rh & s.mhi;
        const bool differs = cl != pl || (WIDE && ch != ph);
        if (j > 0 && pvalid && (!valid || differs)) tail |= 1u << (j - 1);
        if (j < kItems) {
            if (valid && (!pvalid || differs)) head |= 1u << j;
            uint32_t gi = 0xFF;
            if (valid) gi = s.g ? (uint32_t)s.g[i] : (uint32_t)((WIDE ? rh : rl) >> 56);
            tag(j, gi);
        }
        pl = cl, ph = ch, pvalid = valid;
    }
}

// ... and their genome bits, for up to 64 genomes
template <bool WIDE>
DD_D void load_items(const SortedView& s, size_t first, uint32_t& head, uint32_t& tail, uint64_t (&bit)[kItems]) {
    load_slots<WIDE>(s, first, head, tail, [&](int j, uint32_t gi) { bit[j] = (gi < (uint32_t)s.n) ? (1ull << gi) : 0ull; });
}

DD_D void thread_summary(uint32_t head, const uint64_t (&bit)[kItems], uint32_t& f, uint64_t& v) {
    f = head != 0;
    v = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if ((head >> j) & 1u) v = 0;
        v |= bit[j];
    }
}

// The front of a chunk of the sorted array, by a whole workgroup: the calling thread's kItems slots from `first` on, and
// the segmented OR-scan of the chunk over them.  (ef, ev): what the runs in front of the thread's slots, inside the chunk,
// have collected; (tf, tv): the chunk's total.  Holds a barrier.
struct ChunkScan {
    size_t first;
    uint32_t head, tail, ef, tf;
    uint64_t bit[kItems], ev, tv;
};
template <bool WIDE>
DD_D void chunk_scan(const SortedView& s, size_t chunk, ChunkScan& c) {
    __shared__ uint32_t sf[kThreads / 64];
    __shared__ uint64_t sv[kThreads / 64];
    uint32_t f;
    uint64_t v;
    c.first = chunk * kChunk + (size_t)threadIdx.x * kItems;
    load_items<WIDE>(s, c.first, c.head, c.tail, c.bit);
    thread_summary(c.head, c.bit, f, v);
    block_seg_scan<kThreads / 64>(f, v, sf, sv, c.ef, c.ev, c.tf, c.tv);
}

// One round of wave aggregation for a histogram with a dominant bin (progressive: most k-mers meet an ordering at its first
// genomes): the first valid lane's index is added once for every lane that holds it, the other lanes add for themselves.
// Called by whole waves.  Worth 3 x to progressive at k = 21 (profiles/exact_schedules.txt).  NOT to be turned into a loop of
// rounds until every lane is served: that form miscounts in one instantiation for a reason still open;
// leave-out and subsets use plain LDS atomics.
DD_D void agg_add(uint32_t* base, uint32_t idx, bool valid) {
    const unsigned long long act = __ballot(valid);
    if (!act) return;
    const int leader = __builtin_ctzll(act);
    const uint32_t v = __shfl(idx, leader);
    const unsigned long long same = __ballot(valid && idx == v);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&base[v], (uint32_t)__builtin_popcountll(same));
    else if (valid && idx != v) atomicAdd(&base[idx], 1u);
}

size_t exact_sched_chunks(size_t count) { return (count + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace dd
