// dd_exact_wide.hip -- the exact union schedules of dd_exact_sched.hip for 65 to 255 genomes, from the same ONE sort per k.
//
// The sort already carries the genome as a byte (0xFF: the slot nothing wrote); only the 64-bit mask behind it stops at 64.
// Here every distinct k-mer gets a ROW of W = ceil(n / 64) <= 4 words (bit g of the row: genome g holds it) and the three
// schedules that have an object path behind them on the host are additive statistics of those rows, with the contract of
// launch_exact_sched: the caller zeroes acc, acc[0] is the number of distinct k-mers, counts add up over chunks, passes and
// bins of the k-mer space.
//
//   wide_summary  per chunk of 2048 sorted slots (the chunk of the narrow form: the scan pieces of dd_exact_runs.h are shared
//                 as they are): the slots are loaded ONCE, then the segmented OR-scan runs once per 64-genome window of the
//                 row -- the slot's bit in window w is 1 << (g - 64 w) where g - 64 w < 64, else 0 -- and leaves one (head
//                 seen, OR of the open run) pair with W words
//   wide_carry    the segmented OR-scan of those pairs, word by word: one carry per chunk and word.  Nothing walks a run.
//   wide_kernel   per chunk: the same W scans, a row leaves at the LAST slot of its run if any of its words is non-zero (tag
//                 0xFF and any tag >= n set no bit: a run of unwritten slots alone never ends, and where they share their run
//                 with a genuine T^k its bits decide alone) into an LDS tile [W][2048], then the accumulator:
//                   pairwise     512 rows at a time transposed into planes [8][2][n] with one __ballot per genome and 64 rows;
//                                thread t owns genome i = t % n and the pairs (i, i + q mod n), q = 0 .. n / 2 -- every
//                                unordered pair once, the index computed, no pair table -- and adds
//                                popcount(plane_i & plane_j) into u32 sums in registers (128 of them at the most); where
//                                n <= 128 the 256 / n thread groups take the plane words in turn
//                   progressive  nested prefix rows of every ordering in LDS, binary search for the first prefix the row
//                                meets, one round of agg_add; orderings in launches of as many as fit 40 KiB
//                   leave-out    the row's lowest set bit -> its group -> does the row lie inside the group's row? one LDS
//                                counter per group, up to 255 groups
// A u32 sum of a workgroup cannot overflow: a workgroup counts no more rows than it reads slots, 2048 * ceil(chunks / grid),
// which is below 2^32 for every array of fewer than 2^40 slots.
#include <algorithm>

#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"
#include "dd_exact_runs.h"

namespace dd {
namespace {

constexpr int kWideMaxWords = 4;                                   // 64-genome windows of a row
constexpr int kPlaneWords = 8, kPlaneRows = 64 * kPlaneWords;     // pairwise: rows of the tile transposed at a time
constexpr int kWideStaticLds = 256;                                // wide_kernel's own LDS: the scans' wave totals, the counter
constexpr int kWideOrderLds = 40 << 10;                            // progressive: prefix rows + histogram of one launch

struct WideArgs {
    int n;
    int norder;                 // progressive: orderings of this launch
    int ngroups;                // leave-out
    const uint64_t* table;      // progressive: prefix rows [norder][n][W]; leave-out: group of bit [256], group rows [ngroups][W]
    unsigned long long* acc;    // [0] = M (rows seen), then the schedule's counts
    int add_m;
};

// the bit of genome gi in window w of a row (gi outside the window, 0xFFFF included: none)
DD_D uint64_t window_bit(uint32_t gi, int w) {
    const uint32_t b = gi - 64u * (uint32_t)w;
    return b < 64u ? (1ull << b) : 0ull;
}

// The front of a chunk, by a whole workgroup: the calling thread's kItems slots -- loaded once -- and the segmented OR-scan
// of the chunk over them once per window.  (ef, ev[]): what the runs in front of the thread's slots, inside the chunk, have
// collected; (tf, tv[]): the chunk's total.  Holds W barriers; every window has wave totals of its own, so no scan waits
// for the readers of the one before.
template <int W>
struct RowScan {
    size_t first;
    uint32_t head, tail, ef, tf;
    uint32_t gi[kItems];        // the slot's genome, 0xFFFF where it sets no bit
    uint64_t ev[W], tv[W];
};
template <bool WIDE, int W>
DD_D void row_scan(const SortedView& s, size_t chunk, RowScan<W>& c) {
    __shared__ uint32_t sf[W][kThreads / 64];
    __shared__ uint64_t sv[W][kThreads / 64];
    c.first = chunk * kChunk + (size_t)threadIdx.x * kItems;
    load_slots<WIDE>(s, c.first, c.head, c.tail, [&](int j, uint32_t gi) { c.gi[j] = gi < (uint32_t)s.n ? gi : 0xFFFFu; });
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint64_t bit[kItems], v;
        uint32_t f;
#pragma unroll
        for (int j = 0; j < kItems; ++j) bit[j] = window_bit(c.gi[j], w);
        thread_summary(c.head, bit, f, v);
        block_seg_scan<kThreads / 64>(f, v, sf[w], sv[w], c.ef, c.ev[w], c.tf, c.tv[w]);
    }
}
// ... and the runs of the chunk: f(row, ends) for each of the thread's slots, in order, by whole waves -- `row` the OR of
// the slot's run so far, the part in the chunks in front (carry [chunk][W]) included; `ends`: the slot is the last of its
// run and the run holds a genome.
template <bool WIDE, int W, class F>
DD_D void row_runs(const SortedView& s, size_t chunk, const uint64_t* __restrict__ carry, F&& f) {
    RowScan<W> c;
    row_scan<WIDE, W>(s, chunk, c);
    uint64_t run[W];
#pragma unroll
    for (int w = 0; w < W; ++w) run[w] = c.ef ? c.ev[w] : (c.ev[w] | carry[chunk * W + w]);
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        uint64_t any = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if ((c.head >> j) & 1u) run[w] = 0;
            run[w] |= window_bit(c.gi[j], w);
            any |= run[w];
        }
        f(run, ((c.tail >> j) & 1u) && any != 0);
    }
}

template <bool WIDE, int W>
__global__ __launch_bounds__(kThreads) void wide_summary_kernel(SortedView s, uint32_t* __restrict__ sum_f, uint64_t* __restrict__ sum_v) {
    RowScan<W> c;
    row_scan<WIDE, W>(s, blockIdx.x, c);
    if (threadIdx.x == 0) {
        sum_f[blockIdx.x] = c.tf;
#pragma unroll
        for (int w = 0; w < W; ++w) sum_v[(size_t)blockIdx.x * W + w] = c.tv[w];
    }
}

// one workgroup: carry[c][w] = word w of the OR the run open at the end of chunk c-1 has collected
template <int W>
__global__ __launch_bounds__(kCarryThreads) void wide_carry_kernel(const uint32_t* __restrict__ sum_f, const uint64_t* __restrict__ sum_v,
                                                                 size_t nchunks, uint64_t* __restrict__ carry) {
    __shared__ uint32_t sf[W][kCarryThreads / 64];
    __shared__ uint64_t sv[W][kCarryThreads / 64];
    uint64_t run[W];
#pragma unroll
    for (int w = 0; w < W; ++w) run[w] = 0;
    for (size_t base = 0; base < nchunks; base += kCarryThreads) {
        const size_t c = base + threadIdx.x;
        const uint32_t f = c < nchunks ? sum_f[c] : 0u;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = c < nchunks ? sum_v[c * W + w] : 0ull;
            uint32_t ef, tf;
            uint64_t ev, tv;
            block_seg_scan<kCarryThreads / 64>(f, v, sf[w], sv[w], ef, ev, tf, tv);
            if (c < nchunks) carry[c * W + w] = ef ? ev : (run[w] | ev);
            run[w] = tf ? tv : (run[w] | tv);
        }
        __syncthreads();
    }
}

// ---- accumulators: init (LDS state), consume (one tile of rows, word w of row i at tile[w * kChunk + i]; whole workgroup),
// flush (once per workgroup); for the host: lds(n, norder), the dynamic LDS behind the tile
template <int W>
struct AccWidePairwise {
    static constexpr int kSlots = W < kWideMaxWords ? 32 * W + 1 : 128;   // n / 2 + 1 at the most: n <= 64 W, and n <= 255
    uint64_t* planes;   // [kPlaneWords][2][n]: word w of genome i = bit i of rows 64w .. 64w+63 of the batch, the n words twice
                        // in a row: genome i + q mod n lies q words behind genome i, an offset in the instruction, where an
                        // index computed per pair is a register per pair kept over the loop
    int i, part, parts; // this thread's genome; its group of n threads, of 256 / n groups that take the plane words in turn
    uint32_t sum[kSlots];   // slot q: |A_i n A_j|, j = i + q mod n, among the rows this thread has seen
    static size_t lds(int n, int) { return (size_t)kPlaneWords * 2 * n * 8; }
    DD_D void init(const WideArgs& a, uint64_t* dyn) {
        planes = dyn;
        parts = kThreads / a.n > 1 ? kThreads / a.n : 1;
        part = (int)threadIdx.x / a.n, i = (int)threadIdx.x % a.n;
#pragma unroll
        for (int q = 0; q < kSlots; ++q) sum[q] = 0;
    }
    DD_D void consume(const WideArgs& a, const uint64_t* tile, uint32_t cnt) {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int n = a.n;
        for (uint32_t base = 0; base < cnt; base += kPlaneRows) {
            const uint32_t left = (cnt - base + 63) / 64, nw = left < (uint32_t)kPlaneWords ? left : (uint32_t)kPlaneWords;
            for (uint32_t w = wave; w < nw; w += kThreads / 64) {
                const uint32_t r = base + w * 64 + lane;
#pragma unroll
                for (int wd = 0; wd < W; ++wd) {
                    const int nb = n - 64 * wd < 64 ? n - 64 * wd : 64;   // genomes of this window (<= 0: none)
                    const uint64_t m = r < cnt ? tile[wd * kChunk + r] : 0ull;
                    uint64_t mine = 0;
                    for (int b = 0; b < nb; ++b) {
                        const uint64_t word = __ballot((m >> b) & 1ull);
                        if ((int)lane == b) mine = word;
                    }
                    if ((int)lane < nb) planes[(size_t)w * 2 * n + 64 * wd + lane] = planes[(size_t)w * 2 * n + n + 64 * wd + lane] = mine;
                }
            }
            __syncthreads();
            if (part < parts)
                for (uint32_t w = part; w < nw; w += parts) {
                    const uint64_t* p = planes + (size_t)w * 2 * n + i;   // (p[q]: genome i + q mod n, q a constant of the code)
                    const uint64_t mine = p[0];
#pragma unroll
                    for (int q = 0; q < kSlots; ++q)
                        if (2 * q <= n) sum[q] += (uint32_t)__builtin_popcountll(mine & p[q]);
                }
            __syncthreads();
        }
    }
    DD_D void flush(const WideArgs& a) {
        const int n = a.n;
        if (part >= parts) return;
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
            if (2 * q > n || !sum[q]) continue;
            if (2 * q == n && 2 * i >= n) continue;   // (n even: the pairs half way round come up twice, from either end)
            const int j = i + q >= n ? i + q - n : i + q;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            atomicAdd(&a.acc[(size_t)1 + (size_t)lo * n - (size_t)lo * (lo - 1) / 2 + (size_t)(hi - lo)], (unsigned long long)sum[q]);
        }
    }
};

template <int W>
struct AccWideProgressive {
    uint64_t* prefix;   // [norder][n][W]
    uint32_t* hist;     // [norder][n]: k-mers whose first genome in ordering o stands at position j
    static size_t lds(int n, int norder) { return (size_t)norder * n * (8 * W + 4) + 16; }
    DD_D void init(const WideArgs& a, uint64_t* dyn) {
        prefix = dyn;
        hist = reinterpret_cast<uint32_t*>(dyn + (size_t)a.norder * a.n * W);
        for (int i = threadIdx.x; i < a.norder * a.n * W; i += kThreads) prefix[i] = a.table[i];
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads) hist[i] = 0;
    }
    DD_D void consume(const WideArgs& a, const uint64_t* tile, uint32_t cnt) {
        for (uint32_t base = 0; base < cnt; base += kThreads) {
            const uint32_t i = base + threadIdx.x;
            const bool valid = i < cnt;
            uint64_t row[W];
#pragma unroll
            for (int w = 0; w < W; ++w) row[w] = valid ? tile[w * kChunk + i] : 0ull;
            for (int o = 0; o < a.norder; ++o) {
                const uint64_t* p = prefix + (size_t)o * a.n * W;
                int lo = 0, hi = a.n - 1;   // (the last prefix holds every genome: it meets any row)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    uint64_t meets = 0;
#pragma unroll
                    for (int w = 0; w < W; ++w) meets |= row[w] & p[(size_t)mid * W + w];
                    if (meets) hi = mid;
                    else lo = mid + 1;
                }
                agg_add(hist + (size_t)o * a.n, (uint32_t)lo, valid);
            }
        }
    }
    DD_D void flush(const WideArgs& a) {
        for (int i = threadIdx.x; i < a.norder * a.n; i += kThreads)
            if (hist[i]) atomicAdd(&a.acc[1 + i], (unsigned long long)hist[i]);
    }
};

template <int W>
struct AccWideLeaveOut {
    uint64_t* grow;     // [ngroups][W]: the groups' rows
    int32_t* gob;       // [256] group of bit, -1: never left out
    uint32_t* excl;     // [256] k-mers only group g holds
    static size_t lds(int, int) { return (size_t)256 * W * 8 + 256 * 4 + 256 * 4; }
    DD_D void init(const WideArgs& a, uint64_t* dyn) {
        grow = dyn;
        gob = reinterpret_cast<int32_t*>(dyn + 256 * W);
        excl = reinterpret_cast<uint32_t*>(gob + 256);
        gob[threadIdx.x] = (int32_t)a.table[threadIdx.x];   // (kThreads = 256: one bit each)
        excl[threadIdx.x] = 0;
        for (int i = threadIdx.x; i < a.ngroups * W; i += kThreads) grow[i] = a.table[256 + i];
    }
    DD_D void consume(const WideArgs&, const uint64_t* tile, uint32_t cnt) {
        for (uint32_t i = threadIdx.x; i < cnt; i += kThreads) {
            uint64_t row[W];
            int bit = -1;
#pragma unroll
            for (int w = W - 1; w >= 0; --w) {
                row[w] = tile[w * kChunk + i];
                if (row[w]) bit = 64 * w + __builtin_ctzll(row[w]);
            }
            const int32_t g = bit >= 0 ? gob[bit] : -1;
            if (g < 0) continue;
            uint64_t outside = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) outside |= row[w] & ~grow[(size_t)g * W + w];
            if (!outside) atomicAdd(&excl[g], 1u);
        }
    }
    DD_D void flush(const WideArgs& a) {
        if ((int)threadIdx.x < a.ngroups && excl[threadIdx.x]) atomicAdd(&a.acc[1 + threadIdx.x], (unsigned long long)excl[threadIdx.x]);
    }
};

template <bool WIDE, int W, class Acc>
__global__ __launch_bounds__(kThreads) void wide_kernel(SortedView s, const uint64_t* __restrict__ carry, size_t nchunks, WideArgs a) {
    extern __shared__ uint64_t dyn[];
    __shared__ uint32_t cnt;
    uint64_t* tile = dyn;   // [W][kChunk]: a chunk has no more run ends than slots
    Acc acc;
    acc.init(a, dyn + (size_t)W * kChunk);
    unsigned long long seen = 0;   // (thread 0: rows of this workgroup)
    for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (threadIdx.x == 0) cnt = 0;   // (the scans' barriers publish it, and the init)
        row_runs<WIDE, W>(s, chunk, carry, [&](const uint64_t (&run)[W], bool ends) {
            const uint32_t at = wave_append(ends, &cnt);
            if (ends) {
#pragma unroll
                for (int w = 0; w < W; ++w) tile[w * kChunk + at] = run[w];
            }
        });
        __syncthreads();
        const uint32_t have = cnt;
        if (threadIdx.x == 0) seen += have;
        acc.consume(a, tile, have);
        __syncthreads();
    }
    __syncthreads();
    acc.flush(a);
    if (threadIdx.x == 0 && a.add_m && seen) atomicAdd(&a.acc[0], seen);
}

// f(std::integral_constant<int, W>)
template <class F>
void dispatch_words(int words, const F& f) {
    switch (words) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

template <template <int> class Acc, bool WIDE, int W>
void launch_wide_kernel(const SortedView& v, const uint64_t* carry, size_t nchunks, const WideArgs& a, hipStream_t st) {
    const size_t dyn = (size_t)W * kChunk * 8 + Acc<W>::lds(a.n, a.norder);
    // persistent workgroups (the accumulators flush once each): as many as the CUs hold at this much LDS, 4 per CU at most
    const size_t per_cu = std::min<size_t>(4, std::max<size_t>(1, ((size_t)160 << 10) / (dyn + kWideStaticLds)));
    const unsigned grid = (unsigned)std::min<size_t>(nchunks, 256 * per_cu);
    launch_full_lds<wide_kernel<WIDE, W, Acc<W>>, kWideStaticLds>(dim3(grid), dim3(kThreads), dyn, st, v, carry, nchunks, a);
}

}  // namespace

int exact_wide_words(int n) { return (n + 63) / 64; }

size_t exact_wide_acc_words(const ExactWide& s) {
    const size_t n = (size_t)s.n;
    return 1 + (s.kind == kSchedPairwise ? n * (n + 1) / 2 : s.kind == kSchedProgressive ? (size_t)s.norder * n : (size_t)s.ngroups);
}

// per chunk: flag (u32), open-run OR and carry (four u64 each, whatever the row's width)
size_t exact_wide_scratch_bytes(size_t count) { return exact_sched_chunks(count) * (4 + 16 * kWideMaxWords) + 512; }

hipError_t launch_exact_wide(const ExactSorted& sorted, size_t count, int k, const ExactWide& s, void* scratch, hipStream_t st) {
    if (!count) return hipSuccess;
    if (s.n < 1 || s.n > 255) return hipErrorInvalidValue;
    const int words = exact_wide_words(s.n);
    const size_t nchunks = exact_sched_chunks(count);
    uint64_t* sum_v = static_cast<uint64_t*>(scratch);
    uint64_t* carry = sum_v + nchunks * words;
    uint32_t* sum_f = reinterpret_cast<uint32_t*>(carry + nchunks * words);
    const KeyMasks km = key_masks(k);
    const SortedView v{sorted.lo, sorted.hi, sorted.g, km.lo, km.hi, count, s.n};
    dispatch_words(words, [&](auto wc) {
        constexpr int W = decltype(wc)::value;
        dispatch_bool(k > 32, [&](auto wd) {
            constexpr bool WIDE = decltype(wd)::value;
            hipLaunchKernelGGL((wide_summary_kernel<WIDE, W>), dim3((unsigned)nchunks), dim3(kThreads), 0, st, v, sum_f, sum_v);
            hipLaunchKernelGGL(wide_carry_kernel<W>, dim3(1), dim3(kCarryThreads), 0, st, sum_f, sum_v, nchunks, carry);
            // progressive takes its orderings in batches that fit the LDS of a launch
            const bool by_order = s.kind == kSchedProgressive;
            const int items = by_order ? s.norder : 1, per = by_order ? std::max(1, kWideOrderLds / (s.n * (8 * W + 4))) : 1;
            for (int o0 = 0; o0 < items; o0 += per) {
                WideArgs a{s.n, 0, s.ngroups, s.table, s.acc, o0 == 0};
                if (by_order) {
                    a.norder = std::min(per, items - o0);
                    a.table = s.table + (size_t)o0 * s.n * W;
                    a.acc = s.acc + (size_t)o0 * s.n;   // (acc[0] of a later launch is never written: add_m = 0)
                }
                if (s.kind == kSchedPairwise) launch_wide_kernel<AccWidePairwise, WIDE, W>(v, carry, nchunks, a, st);
                else if (by_order) launch_wide_kernel<AccWideProgressive, WIDE, W>(v, carry, nchunks, a, st);
                else launch_wide_kernel<AccWideLeaveOut, WIDE, W>(v, carry, nchunks, a, st);
            }
        });
    });
    return hipGetLastError();
}

}  // namespace dd
