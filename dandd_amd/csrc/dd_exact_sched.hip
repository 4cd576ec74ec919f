// dd_exact_sched.hip -- exact union schedules from ONE sort of the universe per k.
//
// The exact counterparts of dd_pairwise / dd_progressive / dd_leave_out / dd_subsets.  Every k-mer occurrence of all n
// genomes is extracted with the index of its genome (dd_exact.hip, TAG), radix-sorted by the k-mer, and the sorted
// run of each distinct k-mer is OR-ed into a 64-bit MEMBERSHIP MASK (bit i: genome i holds it).  Every schedule is an
// additive statistic of those masks, so the masks never reach HBM (but for the stream, below): a workgroup reduces a chunk of the sorted array
// into an LDS tile of masks and hands the tile to the schedule's accumulator, whose u64 counts add up over chunks,
// passes and bins of the k-mer space.
//
//   sort          launch_exact_sort_tagged: the sort of dd_exact.hip with the genome carried along
//   sched_summary one (head seen, OR of the open run) pair per chunk of 2048 sorted slots
//   sched_carry   segmented OR-scan of those pairs: what the run that crosses into a chunk has collected before it.
//                 A run may be billions of slots long (poly-A); nothing here ever walks one.
//   sched_kernel  per chunk: segmented OR-scan of the slots (registers + wave shuffles), a mask leaves at the LAST
//                 slot of its run and only if it is non-zero -- the slots the single-pass layout never wrote carry
//                 genome 0xFF, set no bit, and share their run with a genuine T^k whose bits then decide alone --
//                 into the LDS tile; then the accumulator:
//                   pairwise     64 masks x 64 bits transposed per wave with one __ballot per genome, plane words in LDS,
//                                every thread owns (i, j) pairs and adds popcount(plane_i & plane_j) in registers
//                   progressive  nested prefix masks in LDS, binary search for the first prefix that meets the mask
//                   leave-out    lowest set bit -> its group -> is the mask inside the group? one counter per group
//                   subsets      histogram of the masks over 2^n bins in LDS (u32; n = 16: two halves by the top bit, on
//                                alternate workgroups)
//                 and the intersection schedules, which ask whether a mask CONTAINS a set and how many bits it has:
//                   spectrum     popcount(mask) over n + 1 bins in LDS; bins 1 and n (where related genomes put almost
//                                every mask) are counted in registers and added once at the flush
//                   core-progressive  the prefix masks of progressive; binary search for the LAST prefix the mask contains;
//                                the full mask is the last bin of every ordering and is counted once, in a register
//                   select       (all, none) pairs in LDS; a thread owns up to 4 queries and a stripe of the tile and
//                                counts its hits in registers
//                 and the one that is no statistic: a walk that picks by the masks of EVERY k at once (dd_exact_greedy.hip)
//                 needs them to outlive their sort
//                   stream       the tile appended to a store in HBM, 8 bytes per distinct k-mer, at a position reserved
//                                with one atomicAdd per tile
//                 and the one that asks nothing in advance:
//                   patterns     the distinct masks with their multiplicities: a hash table of the workgroup in LDS that
//                                leaves for HBM as (mask, count) pairs when it is full and at the end; the pairs of a pass are
//                                sorted, reduced and merged into a running table by dd_exact_patterns.hip
//   emit_kernel   (at the end of this file) sched_kernel's sibling for the selected k-mers themselves: no accumulator, the keys
//                 and masks of the runs that match a query leave for HBM; launch_exact_emit_order then puts them in key order
#include <algorithm>

#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"
#include "dd_exact_runs.h"

namespace dd {
namespace {

constexpr size_t kStaticLds = (size_t)kChunk * 8 + 128;   // sched_kernel's own LDS: the tile of masks, the scan's wave totals
constexpr int kPairSlots = 9;   // ceil(64 * 65 / 2 / 256): (i, j) pairs a thread of the pairwise accumulator owns
constexpr int kSelectSlots = 4, kSelectBatch = kSelectSlots * kThreads;   // queries a thread owns; queries of one select launch

// (the view of the sorted array, a thread's slots, the segmented OR-scan and chunk_scan, the front of a chunk: dd_exact_runs.h,
// shared with the rows of dd_exact_wide.hip)
// The runs of a chunk behind chunk_scan: f(slot, run, ends) for each of the thread's slots, in order, by whole waves -- `run` the
// OR of the slot's run so far, the part in the chunks in front (carry) included; `ends`: the slot is the last of its run and
// the run holds a genome.  The slots the single-pass layout never wrote set no bit: a run of them alone never ends.
template <bool WIDE, class F>
DD_D void chunk_runs(const SortedView& s, size_t chunk, const uint64_t* __restrict__ carry, F&& f) {
    ChunkScan c;
    chunk_scan<WIDE>(s, chunk, c);
    uint64_t run = c.ef ? c.ev : (c.ev | carry[chunk]);
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if ((c.head >> j) & 1u) run = 0;
        run |= c.bit[j];
        f(c.first + j, run, ((c.tail >> j) & 1u) && run != 0);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void sched_summary_kernel(SortedView s, uint32_t* __restrict__ sum_f,
                                                               uint64_t* __restrict__ sum_v) {
    ChunkScan c;
    chunk_scan<WIDE>(s, blockIdx.x, c);
    if (threadIdx.x == 0) sum_f[blockIdx.x] = c.tf, sum_v[blockIdx.x] = c.tv;
}

// one workgroup: carry[c] = the OR the run open at the end of chunk c-1 has collected (chunk c uses it for the slots in
// front of its first head)
__global__ __launch_bounds__(kCarryThreads) void sched_carry_kernel(const uint32_t* __restrict__ sum_f,
                                                                  const uint64_t* __restrict__ sum_v, size_t nchunks,
                                                                  uint64_t* __restrict__ carry) {
    __shared__ uint32_t sf[kCarryThreads / 64];
    __shared__ uint64_t sv[kCarryThreads / 64];
    uint64_t run = 0;   // (value of everything before this tile; its flag is never needed)
    for (size_t base = 0; base < nchunks; base += kCarryThreads) {
        const size_t c = base + threadIdx.x;
        const uint32_t f = c < nchunks ? sum_f[c] : 0u;
        const uint64_t v = c < nchunks ? sum_v[c] : 0ull;
        uint32_t ef, tf;
        uint64_t ev, tv;
        block_seg_scan<kCarryThreads / 64>(f, v, sf, sv, ef, ev, tf, tv);
        if (c < nchunks) carry[c] = ef ? ev : (run | ev);
        run = tf ? tv : (run | tv);
        __syncthreads();
    }
}

struct SchedArgs {
    int n;
    int norder;                       // progressive, core-progressive: orderings of this launch; select: its queries
    int ngroups;                      // leave-out
    const uint64_t* table;            // progressive, core-progressive: prefix masks [norder][n]; leave-out: group of bit [64],
                                      // group masks [ngroups]; select: (all, none) [norder][2]
    unsigned long long* acc;          // [0] = M (masks seen), then the schedule's counts
    int add_m;
    int slices;                       // subsets, n = 16: workgroup w counts the masks whose top bit is w % 2 (every chunk is reduced twice)
    uint64_t* store;                  // stream: where the masks go, the device cursor they are reserved on, the word a tile
    unsigned long long* cursor;       //   that would pass `cap` masks sets
    unsigned long long* overflow;
    unsigned long long cap;
    unsigned long long* counts;       // patterns: the counts beside the masks in `store` (norder: the slots of the LDS table)
    unsigned long long* pstats;       // patterns: [0] += flushes a full table forced, [1] += masks that left on their own
};

// ---- accumulators: init (LDS state), consume (one tile of masks; whole workgroup), flush (once per workgroup) ----
// and, for the host: lds(n, norder), the dynamic LDS init carves, and words(n, norder, ngroups), the counts behind acc[0]
struct AccSubsets {
    uint32_t* hist;     // [2^min(n, 15)]: the bins of this workgroup's slice
    int bits;
    static size_t lds(int n, int) { return (size_t)4 << std::min(n, kExactSubsetsLdsN); }
    static size_t words(int n, int, int) { return (size_t)1 << n; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        bits = a.n < kExactSubsetsLdsN ? a.n : kExactSubsetsLdsN;
        hist = reinterpret_cast<uint32_t*>(dyn);
        for (uint32_t b = threadIdx.x; b < (1u << bits); b += kThreads) hist[b] = 0;
    }
    DD_D void consume(const SchedArgs&, const uint64_t* tile, uint32_t cnt, uint32_t slice) {
        for (uint32_t base = 0; base < cnt; base += kThreads) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t m = i < cnt ? (uint32_t)tile[i] : 0u;
            if (i < cnt && (m >> bits) == slice) atomicAdd(&hist[m & ((1u << bits) - 1u)], 1u);
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t slice) {
        for (uint32_t b = threadIdx.x; b < (1u << bits); b += kThreads)
            if (hist[b]) atomicAdd(&a.acc[1 + ((size_t)slice << bits) + b], (unsigned long long)hist[b]);
    }
};

struct AccLeaveOut {
    uint64_t* gmask;    // [64]
    int32_t* gob;       // [64] group of bit, -1: never left out
    uint32_t* excl;     // [64] k-mers only group g holds
    static size_t lds(int, int) { return 64 * 8 + 64 * 4 + 64 * 4; }
    static size_t words(int, int, int ngroups) { return (size_t)ngroups; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        gmask = dyn;
        gob = reinterpret_cast<int32_t*>(dyn + 64);
        excl = reinterpret_cast<uint32_t*>(dyn + 96);
        if (threadIdx.x < 64) {
            gob[threadIdx.x] = (int32_t)a.table[threadIdx.x];
            gmask[threadIdx.x] = (int)threadIdx.x < a.ngroups ? a.table[64 + threadIdx.x] : 0ull;
            excl[threadIdx.x] = 0;
        }
    }
    DD_D void consume(const SchedArgs&, const uint64_t* tile, uint32_t cnt, uint32_t) {
        for (uint32_t base = 0; base < cnt; base += kThreads) {
            const uint32_t i = base + threadIdx.x;
            const uint64_t m = i < cnt ? tile[i] : 0ull;
            int32_t g = -1;
            if (m) g = gob[__builtin_ctzll(m)];
            const bool only = g >= 0 && (m & ~gmask[g]) == 0;
            if (only) atomicAdd(&excl[g], 1u);
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        if ((int)threadIdx.x < a.ngroups && excl[threadIdx.x]) atomicAdd(&a.acc[1 + threadIdx.x], (unsigned long long)excl[threadIdx.x]);
    }
};

struct AccProgressive {
    uint64_t* prefix;   // [norder][n]
    uint32_t* hist;     // [norder][n]: k-mers whose first genome in ordering o stands at position j
    static size_t lds(int n, int norder) { return (size_t)norder * n * 12 + 16; }
    static size_t words(int n, int norder, int) { return (size_t)norder * n; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        prefix = dyn;
        hist = reinterpret_cast<uint32_t*>(dyn + (size_t)a.norder * a.n);
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads) prefix[i] = a.table[i], hist[i] = 0;
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        for (uint32_t base = 0; base < cnt; base += kThreads) {
            const uint32_t i = base + threadIdx.x;
            const bool valid = i < cnt;
            const uint64_t m = valid ? tile[i] : 0ull;
            for (int o = 0; o < a.norder; ++o) {
                const uint64_t* p = prefix + (size_t)o * a.n;
                int lo = 0, hi = a.n - 1;   // (the last prefix holds every genome: it meets any mask)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (m & p[mid]) hi = mid;
                    else lo = mid + 1;
                }
                agg_add(hist + (size_t)o * a.n, (uint32_t)lo, valid);
            }
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads)
            if (hist[i]) atomicAdd(&a.acc[1 + i], (unsigned long long)hist[i]);
    }
};

struct AccPairwise {
    uint64_t* planes;   // [kChunk / 64][n]: word w of genome i = bit i of masks 64w .. 64w+63 of the tile
    uint8_t *pi, *pj;   // pair p = (pi[p], pj[p]), i <= j
    int npairs;
    unsigned long long sum[kPairSlots];
    static size_t lds(int n, int) { return (size_t)(kChunk / 64) * n * 8 + (size_t)n * (n + 1) + 16; }
    static size_t words(int n, int, int) { return (size_t)n * (n + 1) / 2; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        planes = dyn;
        pi = reinterpret_cast<uint8_t*>(dyn + (size_t)(kChunk / 64) * a.n);
        npairs = a.n * (a.n + 1) / 2;
        pj = pi + npairs;
        for (int i = threadIdx.x; i < a.n; i += kThreads)
            for (int j = i; j < a.n; ++j) {
                const int p = i * a.n - i * (i - 1) / 2 + (j - i);
                pi[p] = (uint8_t)i, pj[p] = (uint8_t)j;
            }
#pragma unroll
        for (int q = 0; q < kPairSlots; ++q) sum[q] = 0;
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        const uint32_t lane = threadIdx.x & 63, nwords = (cnt + 63) / 64;
        for (uint32_t w = threadIdx.x >> 6; w < nwords; w += kThreads / 64) {
            const uint32_t i = w * 64 + lane;
            const uint64_t m = i < cnt ? tile[i] : 0ull;
            uint64_t mine = 0;
            for (int b = 0; b < a.n; ++b) {
                const uint64_t word = __ballot((m >> b) & 1ull);
                if ((int)lane == b) mine = word;
            }
            if ((int)lane < a.n) planes[(size_t)w * a.n + lane] = mine;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPairSlots; ++q) {
            const int p = q * kThreads + threadIdx.x;
            if (p < npairs) {
                const uint64_t *a0 = planes + pi[p], *a1 = planes + pj[p];
                uint32_t c = 0;
                for (uint32_t w = 0; w < nwords; ++w) c += __builtin_popcountll(a0[(size_t)w * a.n] & a1[(size_t)w * a.n]);
                sum[q] += c;
            }
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
#pragma unroll
        for (int q = 0; q < kPairSlots; ++q) {
            const int p = q * kThreads + threadIdx.x;
            if (p < npairs && sum[q]) atomicAdd(&a.acc[1 + p], sum[q]);
        }
    }
};

struct AccSpectrum {
    uint32_t* bins;     // [65]: k-mers held by exactly j genomes
    uint32_t one, all;  // this thread's masks of 1 and of n bits: the two bins related genomes fill, kept off the LDS atomics
    static size_t lds(int, int) { return 65 * 4 + 12; }
    static size_t words(int n, int, int) { return (size_t)n + 1; }
    DD_D void init(const SchedArgs&, uint64_t* dyn) {
        bins = reinterpret_cast<uint32_t*>(dyn);
        if (threadIdx.x <= 64) bins[threadIdx.x] = 0;
        one = all = 0;
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        for (uint32_t i = threadIdx.x; i < cnt; i += kThreads) {
            const int pc = __builtin_popcountll(tile[i]);
            if (pc == a.n) ++all;
            else if (pc == 1) ++one;
            else atomicAdd(&bins[pc], 1u);
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        if (all) atomicAdd(&bins[a.n], all);
        if (one) atomicAdd(&bins[1], one);
        __syncthreads();
        if ((int)threadIdx.x <= a.n && bins[threadIdx.x]) atomicAdd(&a.acc[1 + threadIdx.x], (unsigned long long)bins[threadIdx.x]);
    }
};

struct AccCoreProgressive {
    uint64_t* prefix;   // [norder][n]
    uint32_t* hist;     // [norder][n]: k-mers that hold genomes 0..j of ordering o and not genome j+1
    uint32_t* fulls;    // [1]: the workgroup's full masks
    uint32_t full;      // this thread's full masks: position n-1 of every ordering
    static size_t lds(int n, int norder) { return (size_t)norder * n * 12 + 16; }
    static size_t words(int n, int norder, int) { return (size_t)norder * n; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        prefix = dyn;
        hist = reinterpret_cast<uint32_t*>(dyn + (size_t)a.norder * a.n);
        fulls = hist + (size_t)a.norder * a.n;
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads) prefix[i] = a.table[i], hist[i] = 0;
        if (threadIdx.x == 0) *fulls = 0;
        full = 0;
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        const uint64_t every = a.n == 64 ? ~0ull : ((1ull << a.n) - 1ull);
        for (uint32_t base = 0; base < cnt; base += kThreads) {
            const uint32_t i = base + threadIdx.x;
            const uint64_t m = i < cnt ? tile[i] : 0ull;
            const bool search = m != 0 && m != every;
            full += m == every;
            for (int o = 0; o < a.norder; ++o) {
                const uint64_t* p = prefix + (size_t)o * a.n;
                const bool valid = search && (m & p[0]) == p[0];   // (without the ordering's first genome: in no core)
                int lo = 0, hi = a.n - 1;
                if (valid)
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if ((m & p[mid]) == p[mid]) lo = mid;
                        else hi = mid - 1;
                    }
                agg_add(hist + (size_t)o * a.n, (uint32_t)lo, valid);
            }
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        if (full) atomicAdd(fulls, full);
        __syncthreads();
        const uint32_t f = *fulls;
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads) {
            const uint32_t h = hist[i] + ((i % a.n) == a.n - 1 ? f : 0u);
            if (h) atomicAdd(&a.acc[1 + i], (unsigned long long)h);
        }
    }
};

struct AccSelect {
    uint64_t* pair;     // [norder][2]: (all, none)
    uint32_t* hits;     // [norder]
    uint32_t width;     // threads that share one stripe of the tile: a power of two >= the queries, kThreads at most
    uint32_t c[kSelectSlots];   // hits of queries (threadIdx.x % width) + r * kThreads among the masks of this thread's stripe
    static size_t lds(int, int norder) { return (size_t)norder * 20 + 16; }
    static size_t words(int, int norder, int) { return (size_t)norder; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        pair = dyn;
        hits = reinterpret_cast<uint32_t*>(dyn + 2 * (size_t)a.norder);
        for (int i = threadIdx.x; i < 2 * a.norder; i += kThreads) pair[i] = a.table[i];
        for (int i = threadIdx.x; i < a.norder; i += kThreads) hits[i] = 0;
        width = 1;
        while (width < (uint32_t)a.norder && width < (uint32_t)kThreads) width <<= 1;
#pragma unroll
        for (int r = 0; r < kSelectSlots; ++r) c[r] = 0;
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        const uint32_t q0 = threadIdx.x & (width - 1), step = kThreads / width;
        const int rounds = (a.norder + kThreads - 1) / kThreads;
        uint64_t all[kSelectSlots], none[kSelectSlots];
#pragma unroll
        for (int r = 0; r < kSelectSlots; ++r) {
            const uint32_t q = q0 + (uint32_t)r * kThreads;
            const bool live = q < (uint32_t)a.norder;   // (all = none = ~0 matches no mask)
            all[r] = live ? pair[2 * q] : ~0ull;
            none[r] = live ? pair[2 * q + 1] : ~0ull;
        }
        for (uint32_t i = threadIdx.x / width; i < cnt; i += step) {
            const uint64_t m = tile[i];
#pragma unroll
            for (int r = 0; r < kSelectSlots; ++r)
                if (r < rounds) c[r] += mask_matches(m, all[r], none[r]);
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        const uint32_t q0 = threadIdx.x & (width - 1);
#pragma unroll
        for (int r = 0; r < kSelectSlots; ++r) {
            const uint32_t q = q0 + (uint32_t)r * kThreads;
            if (q < (uint32_t)a.norder && c[r]) atomicAdd(&hits[q], c[r]);
        }
        __syncthreads();
        for (int q = threadIdx.x; q < a.norder; q += kThreads)
            if (hits[q]) atomicAdd(&a.acc[1 + q], (unsigned long long)hits[q]);
    }
};

struct AccStream {
    unsigned long long* at;   // [1]: where this tile goes, from the thread that reserved it to the others (no state: rewritten per tile)
    static size_t lds(int, int) { return 16; }
    static size_t words(int, int, int) { return 0; }
    DD_D void init(const SchedArgs&, uint64_t* dyn) { at = reinterpret_cast<unsigned long long*>(dyn); }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        if (!cnt) return;   // (cnt is the same in every thread)
        if (threadIdx.x == 0) *at = atomicAdd(a.cursor, (unsigned long long)cnt);
        __syncthreads();
        const unsigned long long base = *at;
        if (base + cnt <= a.cap) {
            for (uint32_t i = threadIdx.x; i < cnt; i += kThreads) a.store[base + i] = tile[i];
        } else if (threadIdx.x == 0) {
            *a.overflow = 1ull;
        }
    }
    DD_D void flush(const SchedArgs&, uint32_t) {}
};

// The masks themselves with their multiplicities: an open-addressing table of the workgroup in LDS -- keys the 64-bit masks
// (0 is the empty slot: a zero mask never leaves chunk_runs), counts u32 -- that leaves for HBM as (mask, count) pairs at a
// position reserved with one atomicAdd per flush, as the stream reserves its tiles.  A thread places its masks of a tile by
// linear probing over at most kPatternProbe slots (64-bit LDS compare-and-swap on the key, LDS add on the count).  When some
// thread of the workgroup could not place a mask, the whole workgroup writes the table out and clears it, the masks left over
// are tried once more on the empty table, and one that still finds no slot (more than kPatternProbe of the left-over masks
// share its probe sequence) leaves on its own as (mask, weight): every tile costs one such round at the most, whatever the
// masks are.  The full mask -- where related genomes put most k-mers -- is counted in a register and leaves as one pair per
// workgroup at the flush; of the others, the first live mask of each wave is added once for all the lanes that hold it (one
// round, as agg_add).  A pair stands for at least one mask seen, so a pass writes no more pairs than it has slots.
constexpr int kPatternProbe = 16;
DD_D uint32_t pattern_hash(uint64_t m, int shift) {   // shift = 64 - log2(slots): the product's top bits, which depend on every bit of m
    return (uint32_t)((m * 0x9E3779B97F4A7C15ull) >> shift);
}

struct AccPatterns {
    unsigned long long* keys;   // [slots]
    uint32_t* cnts;             // [slots]
    unsigned long long* fulls;  // [1]: the workgroup's full masks
    unsigned long long* at;     // [1]: where a flush goes
    uint32_t* used;             // [2]: non-empty slots of a flush; the position its writers count on
    uint32_t slots;
    int shift;                  // 64 - log2(slots)
    unsigned long long full;    // this thread's full masks
    static size_t lds(int, int slots) { return (size_t)slots * 12 + 32; }
    static size_t words(int, int, int) { return 0; }
    DD_D void init(const SchedArgs& a, uint64_t* dyn) {
        slots = (uint32_t)a.norder;   // a power of two, 64 at least
        shift = 64 - __builtin_ctz(slots);
        keys = reinterpret_cast<unsigned long long*>(dyn);
        cnts = reinterpret_cast<uint32_t*>(keys + slots);
        fulls = reinterpret_cast<unsigned long long*>(cnts + slots);   // (slots is even: 8-byte aligned)
        at = fulls + 1;
        used = reinterpret_cast<uint32_t*>(at + 1);
        for (uint32_t s = threadIdx.x; s < slots; s += kThreads) keys[s] = 0ull, cnts[s] = 0u;
        if (threadIdx.x == 0) *fulls = 0ull, *at = 0ull, used[0] = used[1] = 0u;
        full = 0;
    }
    DD_D bool insert(uint64_t m, uint32_t weight) {
        const uint32_t h = pattern_hash(m, shift);
        for (int p = 0; p < kPatternProbe; ++p) {
            const uint32_t s = (h + (uint32_t)p) & (slots - 1u);
            unsigned long long was = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (was == 0ull) was = atomicCAS(&keys[s], 0ull, (unsigned long long)m);
            if (was == 0ull || was == m) {
                atomicAdd(&cnts[s], weight);
                return true;
            }
        }
        return false;
    }
    // (mask, count) pairs for HBM at a reserved position; a range that would pass the capacity is not written and says so
    DD_D void put(const SchedArgs& a, unsigned long long pos, uint64_t m, unsigned long long count) {
        a.store[pos] = m, a.counts[pos] = count;
    }
    // the table written out and cleared, by the whole workgroup; holds barriers
    DD_D void spill(const SchedArgs& a) {
        uint32_t mine = 0;
        for (uint32_t s = threadIdx.x; s < slots; s += kThreads) mine += keys[s] != 0ull;
        if (mine) atomicAdd(&used[0], mine);
        __syncthreads();
        const uint32_t total = used[0];
        if (threadIdx.x == 0 && total) *at = atomicAdd(a.cursor, (unsigned long long)total);
        __syncthreads();
        const unsigned long long base = *at;
        const bool room = base + total <= a.cap;
        if (total && !room && threadIdx.x == 0) *a.overflow = 1ull;
        for (uint32_t s0 = 0; s0 < slots; s0 += kThreads) {   // (slots is a multiple of 64: whole waves)
            const uint32_t s = s0 + threadIdx.x;
            const bool live = s < slots && keys[s] != 0ull;
            const uint32_t p = wave_append(live, &used[1]);
            if (live) {
                if (room) put(a, base + p, keys[s], (unsigned long long)cnts[s]);
                keys[s] = 0ull, cnts[s] = 0u;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) used[0] = used[1] = 0u;
        __syncthreads();
    }
    DD_D void consume(const SchedArgs& a, const uint64_t* tile, uint32_t cnt, uint32_t) {
        if (!cnt) return;   // (cnt is the same in every thread)
        const uint64_t every = a.n == 64 ? ~0ull : ((1ull << a.n) - 1ull);
        const int lane = threadIdx.x & 63;
        uint32_t left = 0, weight[kItems];   // bit j: mask j * kThreads + threadIdx.x of the tile found no slot
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const uint32_t i = (uint32_t)j * kThreads + threadIdx.x;
            uint64_t m = i < cnt ? tile[i] : 0ull;
            if (m == every) ++full, m = 0ull;
            // one round of wave aggregation: the first live lane's mask is added once for every lane that holds it
            bool live = m != 0ull;
            weight[j] = 1u;
            const unsigned long long act = __ballot(live);
            if (act) {
                const int leader = __builtin_ctzll(act);
                const uint64_t v = __shfl((unsigned long long)m, leader);
                const unsigned long long same = __ballot(live && m == v);
                if (lane == leader) weight[j] = (uint32_t)__builtin_popcountll(same);
                else if (m == v) live = false;
            }
            if (live && !insert(m, weight[j])) left |= 1u << j;
        }
        if (!__syncthreads_or(left != 0u)) return;
        // a full table: written out, and the masks left over placed in the empty one, or sent on their own
        if (threadIdx.x == 0) atomicAdd(&a.pstats[0], 1ull);
        spill(a);
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const bool pending = (left >> j) & 1u;
            const uint64_t m = pending ? tile[(uint32_t)j * kThreads + threadIdx.x] : 0ull;
            const bool single = pending && !insert(m, weight[j]);
            const unsigned long long singles = __ballot(single);
            if (singles) {   // (wave_append on the device cursor, with the capacity checked for the wave's range)
                const int leader = __builtin_ctzll(singles);
                const uint32_t nw = (uint32_t)__builtin_popcountll(singles);
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(a.cursor, (unsigned long long)nw), atomicAdd(&a.pstats[1], (unsigned long long)nw);
                base = __shfl(base, leader);
                if (base + nw <= a.cap) {
                    if (single) put(a, base + (unsigned long long)__builtin_popcountll(singles & ((1ull << lane) - 1ull)), m, weight[j]);
                } else if (lane == leader) {
                    *a.overflow = 1ull;
                }
            }
        }
    }
    DD_D void flush(const SchedArgs& a, uint32_t) {
        if (full) atomicAdd(fulls, full);
        __syncthreads();
        if (threadIdx.x == 0 && *fulls) {   // the full mask never entered the table: one pair of the workgroup's own
            const unsigned long long pos = atomicAdd(a.cursor, 1ull);
            if (pos < a.cap) put(a, pos, a.n == 64 ? ~0ull : ((1ull << a.n) - 1ull), *fulls);
            else *a.overflow = 1ull;
        }
        spill(a);
    }
};

template <bool WIDE, class Acc>
__global__ __launch_bounds__(kThreads) void sched_kernel(SortedView s, const uint64_t* __restrict__ carry, size_t nchunks,
                                                       SchedArgs a) {
    extern __shared__ uint64_t dyn[];
    __shared__ uint64_t tile[kChunk];
    __shared__ uint32_t cnt;
    Acc acc;
    acc.init(a, dyn);
    unsigned long long seen = 0;   // (thread 0: masks of this workgroup)
    const uint32_t slice = blockIdx.x % (uint32_t)a.slices;   // (the grid is a multiple of the slices)
    for (size_t chunk = blockIdx.x / (uint32_t)a.slices; chunk < nchunks; chunk += gridDim.x / (uint32_t)a.slices) {
        if (threadIdx.x == 0) cnt = 0;   // (the scan's barrier publishes it, and the init)
        chunk_runs<WIDE>(s, chunk, carry, [&](size_t, uint64_t run, bool ends) {
            const uint32_t at = wave_append(ends, &cnt);
            if (ends) tile[at] = run;
        });
        __syncthreads();
        const uint32_t have = cnt;
        if (threadIdx.x == 0 && slice == 0) seen += have;
        acc.consume(a, tile, have, slice);
        __syncthreads();
    }
    __syncthreads();
    acc.flush(a, slice);
    if (threadIdx.x == 0 && a.add_m && seen) atomicAdd(&a.acc[0], seen);
}

// orderings one progressive or core-progressive launch takes: prefix masks + histogram within 40 KiB of LDS
int max_orderings(int n) { return std::max(1, (40 << 10) / (12 * n)); }

// the one place that maps a kSched* to its accumulator: f(AccTag<Acc>)
template <class Acc>
struct AccTag {
    using type = Acc;
};
template <class F>
auto with_acc(int kind, const F& f) {
    switch (kind) {
        case kSchedPairwise: return f(AccTag<AccPairwise>{});
        case kSchedProgressive: return f(AccTag<AccProgressive>{});
        case kSchedLeaveOut: return f(AccTag<AccLeaveOut>{});
        case kSchedSpectrum: return f(AccTag<AccSpectrum>{});
        case kSchedCoreProgressive: return f(AccTag<AccCoreProgressive>{});
        case kSchedSelect: return f(AccTag<AccSelect>{});
        case kSchedStream: return f(AccTag<AccStream>{});
        case kSchedPatterns: return f(AccTag<AccPatterns>{});
        default: return f(AccTag<AccSubsets>{});
    }
}

size_t sched_dyn_lds(int kind, int n, int norder) {
    return with_acc(kind, [&](auto t) { return decltype(t)::type::lds(n, norder); });
}

// What sched_kernel and emit_kernel both stand on: the scratch carved (open-run ORs | carries | flags, one per chunk), the
// view of the sorted array, and the two pre-passes launched.
struct SortedHead {
    SortedView v;
    const uint64_t* carry;   // per chunk: what the run that crosses into it has collected
    size_t nchunks;
};

SortedHead sorted_head(const ExactSorted& sorted, size_t count, int k, int n, void* scratch, hipStream_t st) {
    const size_t nchunks = exact_sched_chunks(count);
    uint64_t* sum_v = static_cast<uint64_t*>(scratch);
    uint64_t* carry = sum_v + nchunks;
    uint32_t* sum_f = reinterpret_cast<uint32_t*>(carry + nchunks);
    const KeyMasks km = key_masks(k);
    const SortedView v{sorted.lo, sorted.hi, sorted.g, km.lo, km.hi, count, n};
    dispatch_bool(k > 32, [&](auto w) {
        hipLaunchKernelGGL(sched_summary_kernel<decltype(w)::value>, dim3((unsigned)nchunks), dim3(kThreads), 0, st, v, sum_f, sum_v);
    });
    hipLaunchKernelGGL(sched_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, sum_f, sum_v, nchunks, carry);
    return SortedHead{v, carry, nchunks};
}

size_t order_temp_bytes(size_t found, int k) { return exact_sort_keys_temp_bytes(found, k, sizeof(uint64_t)); }   // of launch_exact_emit_order's sort

}  // namespace

size_t exact_sched_acc_words(const ExactSched& s) {
    return 1 + with_acc(s.kind, [&](auto t) { return decltype(t)::type::words(s.n, s.norder, s.ngroups); });
}

// per chunk: flag (u32), open-run OR (u64), carry (u64)
size_t exact_sched_scratch_bytes(size_t count) { return exact_sched_chunks(count) * 24 + 512; }

size_t exact_sched_temp_bytes(size_t n, int k) { return exact_sort_keys_temp_bytes(n, k, sizeof(uint8_t)); }

// launch_exact_sort_keys with the genome of tag mode 2 following; only k = 61..64 pay for its second run of each pass.
hipError_t launch_exact_sort_tagged(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, uint8_t* g, uint8_t* g_alt,
                                    size_t n, int k, void* temp, size_t temp_bytes, hipStream_t st, ExactSorted* out) {
    const bool sep = exact_tag_mode(k) == 2;
    const hipError_t e = launch_exact_sort_keys(lo, hi, lo_alt, hi_alt, sep ? g : nullptr, g_alt, sizeof(uint8_t), n, k, temp, temp_bytes, st);
    if (k <= 32) *out = ExactSorted{lo_alt, nullptr, sep ? g_alt : nullptr};
    else if (e == hipSuccess) *out = ExactSorted{lo, hi, sep ? g : nullptr};
    return e;
}

hipError_t launch_exact_sched(const ExactSorted& sorted, size_t count, int k, const ExactSched& s, void* scratch, hipStream_t st) {
    if (!count) return hipSuccess;
    const bool wide = k > 32;
    const SortedHead h = sorted_head(sorted, count, k, s.n, scratch, st);
    // progressive and core-progressive take their orderings, select its queries, in batches that fit the LDS of a launch
    const bool by_order = s.kind == kSchedProgressive || s.kind == kSchedCoreProgressive, by_query = s.kind == kSchedSelect;
    const int items = (by_order || by_query) ? s.norder : 1, per = by_order ? max_orderings(s.n) : (by_query ? kSelectBatch : 1);
    const size_t tstride = by_order ? (size_t)s.n : 2, astride = by_order ? (size_t)s.n : 1;
    for (int o0 = 0; o0 < items; o0 += per) {
        SchedArgs a{s.n, 0, s.ngroups, s.table, s.acc, o0 == 0, 1, s.store, s.cursor, s.overflow, s.cap, s.counts, s.pstats};
        if (s.kind == kSchedPatterns) a.norder = s.norder;
        if (s.kind == kSchedSubsets && s.n > kExactSubsetsLdsN) a.slices = 1 << (s.n - kExactSubsetsLdsN);
        if (by_order || by_query) {
            a.norder = std::min(per, items - o0);
            a.table = s.table + (size_t)o0 * tstride;
            a.acc = s.acc + (size_t)o0 * astride;   // (acc[0] of a later launch is never written: add_m = 0)
        }
        const size_t dyn = sched_dyn_lds(s.kind, s.n, a.norder);
        // persistent workgroups (the accumulators flush once each): as many as the CUs hold at this much LDS, 4 per CU at most
        const size_t per_cu = std::min<size_t>(4, std::max<size_t>(1, ((size_t)160 << 10) / (dyn + kStaticLds)));
        const unsigned grid = (unsigned)(std::min<size_t>(h.nchunks, 256 * per_cu) * a.slices);
        // (every sched_kernel may take the dynamic LDS a CU has left beside the kernel's own: subsets asks for 128 KiB)
        dispatch_bool(wide, [&](auto w) {
            with_acc(s.kind, [&](auto t) {
                launch_full_lds<sched_kernel<decltype(w)::value, typename decltype(t)::type>, kStaticLds>(dim3(grid), dim3(kThreads), dyn, st, h.v, h.carry,
                                                                                                  h.nchunks, a);
            });
        });
    }
    return hipGetLastError();
}

// ---- emit: the selected k-mers themselves -------------------------------------------------------------------------------
// A sibling of sched_kernel behind the same two pre-passes.  The same segmented OR-scan of a chunk; at the last slot of a
// run whose mask is non-zero the mask is tested against the (all, none) pairs in LDS, and the first hit is enough: a k-mer
// that matches several queries leaves once.  A hit stages (lo, hi, mask) in LDS -- the slot's key under mlo / mhi, so the
// genome of tag mode 1 never leaves, and hi only for k > 32 -- at a position from one ballot and one LDS counter per wave,
// as the tile of sched_kernel is filled; the workgroup then reserves its range of the output with ONE atomicAdd on the
// device cursor per chunk and writes it with plain stores.  The cursor keeps counting past `cap`: a range that would pass
// it is not written, and the caller reads from the cursor how many records there were.  Ranges land in the order the
// chunks finish; who wants an order calls launch_exact_emit_order behind the last pass (both callers do).
namespace {

constexpr size_t kEmitStaticLds = 128;   // emit_kernel's own LDS: the scan's wave totals, the counter, the reserved position

template <bool WIDE>
__global__ __launch_bounds__(kThreads) void emit_kernel(SortedView s, const uint64_t* __restrict__ carry, size_t nchunks, ExactEmit a) {
    extern __shared__ uint64_t dyn[];
    __shared__ uint32_t cnt;
    __shared__ unsigned long long at;
    uint64_t* pair = dyn;                          // [nq][2]: (all, none)
    uint64_t* st_mask = dyn + 2 * (size_t)a.nq;    // [kChunk] each: a chunk has no more run ends than slots
    uint64_t* st_lo = st_mask + kChunk;
    uint64_t* st_hi = st_lo + kChunk;              // WIDE only
    for (int i = threadIdx.x; i < 2 * a.nq; i += kThreads) pair[i] = a.table[i];
    for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x == 0) cnt = 0;   // (the scan's barrier publishes it, and the pairs)
        chunk_runs<WIDE>(s, chunk, carry, [&](size_t slot, uint64_t run, bool ends) {
            bool hit = false;
            if (ends)
                for (int q = 0; q < a.nq && !hit; ++q) hit = mask_matches(run, pair[2 * q], pair[2 * q + 1]);
            const uint32_t p = wave_append(hit, &cnt);
            if (hit) {   // (a run ends inside the array: load_items sets the bit only behind a valid slot)
                st_mask[p] = run;
                st_lo[p] = s.lo[slot] & s.mlo;
                if (WIDE) st_hi[p] = s.hi[slot] & s.mhi;
            }
        });
        __syncthreads();
        const uint32_t have = cnt;   // (the same in every thread)
        if (have) {
            if (threadIdx.x == 0) at = atomicAdd(a.cursor, (unsigned long long)have);
            __syncthreads();
            const unsigned long long base = at;
            if (base + have <= a.cap)
                for (uint32_t i = threadIdx.x; i < have; i += kThreads) {
                    a.mask[base + i] = st_mask[i];
                    a.lo[base + i] = st_lo[i];
                    if (WIDE) a.hi[base + i] = st_hi[i];
                }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_exact_emit(const ExactSorted& sorted, size_t count, int k, const ExactEmit& e, void* scratch, hipStream_t st) {
    if (!count) return hipSuccess;
    const bool wide = k > 32;
    const SortedHead h = sorted_head(sorted, count, k, e.n, scratch, st);
    // the pairs, then a staging area of kChunk records (all = none = 0 hits every distinct k-mer): 48 KiB + 16 KiB at the most
    const size_t dyn = ((size_t)2 * e.nq + (size_t)(wide ? 3 : 2) * kChunk) * sizeof(uint64_t);
    const size_t per_cu = std::min<size_t>(4, std::max<size_t>(1, ((size_t)160 << 10) / (dyn + kEmitStaticLds)));
    const dim3 g((unsigned)std::min<size_t>(h.nchunks, 256 * per_cu)), t(kThreads);   // persistent workgroups, as launch_exact_sched sizes them
    dispatch_bool(wide, [&](auto w) { launch_full_lds<emit_kernel<decltype(w)::value>, (int)kEmitStaticLds>(g, t, dyn, st, h.v, h.carry, h.nchunks, e); });
    return hipGetLastError();
}

// ---- the emitted records in ascending key order ------------------------------------------------------------------------
// launch_exact_sort_keys over the records, the mask following.  `work`: the other halves of the double buffers (lo, mask[, hi]),
// then the sort's temp.
size_t exact_emit_order_bytes(size_t found, int k) {
    return (size_t)(k > 32 ? 3 : 2) * ((found * sizeof(uint64_t) + 255) / 256 * 256) + order_temp_bytes(found, k);
}

hipError_t launch_exact_emit_order(uint64_t* lo, uint64_t* hi, uint64_t* mask, size_t found, int k, void* work, hipStream_t st,
                                   LocateSet* out) {
    const size_t stride = (found * sizeof(uint64_t) + 255) / 256 * 256;
    char* wb = static_cast<char*>(work);
    uint64_t* lo_alt = reinterpret_cast<uint64_t*>(wb);
    uint64_t* mask_alt = reinterpret_cast<uint64_t*>(wb + stride);
    uint64_t* hi_alt = reinterpret_cast<uint64_t*>(wb + 2 * stride);   // k > 32 only: the temp stands there otherwise
    void* temp = wb + (k > 32 ? 3 : 2) * stride;
    const hipError_t e = launch_exact_sort_keys(lo, hi, lo_alt, hi_alt, mask, mask_alt, sizeof(uint64_t), found, k, temp, order_temp_bytes(found, k), st);
    if (k <= 32) *out = LocateSet{lo_alt, nullptr, mask_alt, found};
    else if (e == hipSuccess) *out = LocateSet{lo, hi, mask, found};
    return e;
}

}  // namespace dd
