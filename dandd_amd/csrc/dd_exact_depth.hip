// dd_exact_depth.hip -- samples that are no leaves, counted against the ordered records of an exact universe: how many TIMES a
// sample holds each k-mer of the universe, binned by depth per genome and per query.
//
// dd_exact_screen.hip keeps a bit per (sample, record), dd_exact_paint.hip and dd_exact_reads.hip count positions per window
// or row of the sample.  Here the counter belongs to the RECORD: behind the same ordered records (a LocateSet) two kernels
// leave, per sample and per row of records -- genome i: the records whose mask has bit i; query q: the records whose mask
// matches pair q --, the histogram of the records' depths and nothing else.
//
//   depth    depth_kernel: screen_kernel's frame -- one thread per 64-token segment of a sample's token stream, one launch
//            unit (gridDim.y) per sample of the round, walk_segment and find_record of dd_exact_walk.h.  An exact hit at
//            record r issues one no-return atomicAdd(&count[s][r], 1u) on the sample's row of `found` 32-bit counters,
//            zeroed by the caller.  No test in front of the add: every hit counts, that is the answer.  A miss issues
//            nothing.  A counter holds the positions of ONE sample, which are fewer than its bytes: the entry refuses a
//            sample of 2^32 bytes or more, so no counter wraps.
//   tally    depth_tally_kernel: the grid runs over (range of the records, sample of the round, tile of rows).  A tile is as
//            many rows as the workgroup's histogram in LDS holds: per row `bins` 32-bit counters, one 64-bit overflow sum
//            and, for a query row, its (all, none) pair.  A wave takes 64 consecutive records, lane l the record 64 g + l,
//            and loads their counters; a group whose counters are all zero is skipped after that one load and one ballot --
//            the kernel touches records with c >= 1 only.
//
// Bin 0 is never accumulated: it is the size of the row less the other bins, and the sizes come from launch_exact_tally
// with no sample at all (dd_exact_screen.hip, used as it is).  A sample of another species would otherwise add every
// record of the universe to bin 0 of every row it lies in; as it is, such a sample costs one counter load per record.
//
// How the tally bins, and why.  A record of depth d adds 1 to hist[row][min(d, bins - 1)] of every row that holds it.  One
// LDS atomic per (record, row) serialises where the lanes of a wave share a bin, and they do in the common cases: a sample
// that is a genome of the universe has depth 1 everywhere, an assembly mostly 1, a read set clusters round its coverage.
// So the wave takes the bin of its first live lane, d0, and `same` = the lanes in that bin (AccPatterns' elect-then-consume
// form, dd_exact_sched.hip); for every row of the tile __ballot(same && the lane's record lies in the row) is consumed whole
// by one popcount and ONE LDS add from one lane.  The lanes outside `same` add singly with LDS atomics: they are spread over
// other bins and collide little.  A loop that elects again until no lane is left would be exact too, but costs a ballot per
// (row, distinct bin of the group) where a read set has twenty distinct bins among 64 records.
// A record with c >= bins - 1 goes to the last bin and adds c - (bins - 1) to its rows' 64-bit overflow sums; the entry
// computes total = sum_d d * hist[d] + overflow, so the common record issues no second add.
// After the last group the workgroup issues one global 64-bit atomicAdd per non-zero LDS counter.  No global atomic is
// issued per record.  Integer sums: the order of arrival does not change them, two calls return identical bytes.
#include <algorithm>
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void depth_kernel(const ExactGenome* __restrict__ samples, int k, LocateSet set, uint32_t* count) {
    const ExactGenome* u = samples + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* mine = count + (unsigned long long)blockIdx.y * set.found;
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long, int, uint64_t ah, uint64_t al, bool) {
        unsigned long long r;
        if (!find_record<WIDE>(set, ah, al, r)) return;
        atomicAdd(mine + r, 1u);   // (r < found: inside the row)
    });
}

constexpr int kDepthTallyThreads = 256;
constexpr size_t kDepthGroupsPerWave = 16;   // record groups a wave should have before another workgroup is worth its flush

// the LDS of a tile of `rows` rows: overflow sums [rows] u64 | pairs [rows][2] u64 | bins [rows][bins] u32
DD_HD size_t depth_tile_bytes(size_t rows, int bins) { return rows * (3 * sizeof(uint64_t) + (size_t)bins * sizeof(uint32_t)); }

__global__ __launch_bounds__(kDepthTallyThreads) void depth_tally_kernel(const uint64_t* __restrict__ mask, unsigned long long found,
                                                                         const uint32_t* __restrict__ count, int n, int nq, int bins,
                                                                         int rows_tile, const uint64_t* __restrict__ table,
                                                                         unsigned long long* __restrict__ hist_out,
                                                                         unsigned long long* __restrict__ over_out) {
    extern __shared__ uint64_t lds[];
    const int nrow = n + nq, row_lo = (int)blockIdx.z * rows_tile, row_hi = row_lo + rows_tile < nrow ? row_lo + rows_tile : nrow;
    const int rows = row_hi - row_lo;                                    // of this tile: >= 1
    const int gen_hi = row_hi < n ? row_hi : n;                          // its genome rows: row_lo .. gen_hi - 1
    const int q_lo = (row_lo > n ? row_lo : n) - n, q_hi = row_hi - n;   // its queries: q_lo .. q_hi - 1 (none: q_hi <= q_lo)
    unsigned long long* over = reinterpret_cast<unsigned long long*>(lds);
    uint64_t* pair = lds + rows_tile;
    uint32_t* bin = reinterpret_cast<uint32_t*>(lds + 3 * (size_t)rows_tile);
    for (int i = threadIdx.x; i < rows; i += kDepthTallyThreads) over[i] = 0;
    for (int i = threadIdx.x; i < 2 * (q_hi - q_lo); i += kDepthTallyThreads) pair[i] = table[2 * (size_t)q_lo + i];
    for (int i = threadIdx.x; i < rows * bins; i += kDepthTallyThreads) bin[i] = 0;
    __syncthreads();
    const uint32_t* mine = count + (unsigned long long)blockIdx.y * found;
    const int lane = threadIdx.x & 63;
    const uint32_t top = (uint32_t)bins - 1;
    const unsigned long long groups = (found + 63) / 64, waves = (unsigned long long)gridDim.x * (kDepthTallyThreads / 64);
    for (unsigned long long g = (unsigned long long)blockIdx.x * (kDepthTallyThreads / 64) + (threadIdx.x >> 6); g < groups; g += waves) {
        const unsigned long long r = g * 64 + lane;
        const uint32_t c = r < found ? mine[r] : 0u;
        const bool live = c != 0;
        const unsigned long long lives = __ballot(live);
        if (!lives) continue;   // (the same in every lane of the wave)
        const uint64_t m = live ? mask[r] : 0ull;
        const uint32_t d = c < top ? c : top, extra = c - d;
        const uint32_t d0 = (uint32_t)__shfl((int)d, __builtin_ctzll(lives));
        const bool same = live && d == d0, single = live && d != d0;
        const bool spill = __ballot(extra != 0) != 0;
        // row `at` of the tile takes the lanes that are `in` it
        const auto take = [&](int at, bool in) {
            const unsigned long long col = __ballot(in && same);
            if (lane == 0 && col) atomicAdd(&bin[at * bins + (int)d0], (uint32_t)__builtin_popcountll(col));
            if (in && single) atomicAdd(&bin[at * bins + (int)d], 1u);
            if (spill && in && extra) atomicAdd(&over[at], (unsigned long long)extra);
        };
        for (int b = row_lo; b < gen_hi; ++b) take(b - row_lo, (m >> b) & 1ull);
        for (int q = q_lo; q < q_hi; ++q) take(n + q - row_lo, live && mask_matches(m, pair[2 * (q - q_lo)], pair[2 * (q - q_lo) + 1]));
    }
    __syncthreads();
    // (bin 0 of every row is still zero: the entry derives it)
    unsigned long long* hist = hist_out + ((unsigned long long)blockIdx.y * nrow + row_lo) * bins;
    for (int i = threadIdx.x; i < rows * bins; i += kDepthTallyThreads)
        if (bin[i]) atomicAdd(&hist[i], (unsigned long long)bin[i]);
    for (int i = threadIdx.x; i < rows; i += kDepthTallyThreads)
        if (over[i]) atomicAdd(&over_out[(unsigned long long)blockIdx.y * nrow + row_lo + i], over[i]);
}

}  // namespace

void launch_exact_depth(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set,
                        uint32_t* count_dev, hipStream_t st) {
    if (ns <= 0 || !max_segments || !set.found) return;
    launch_segment_walk((size_t)ns, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((depth_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, samples_dev, k, set, count_dev);
    });
}

int exact_depth_rows_tile(int bins) { return (int)(kDepthTileBytes / depth_tile_bytes(1, bins)); }

void launch_exact_depth_tally(const LocateSet& set, const uint32_t* count_dev, int ns, int n, int nq, int bins, const uint64_t* table_dev,
                              unsigned long long* hist_dev, unsigned long long* over_dev, hipStream_t st) {
    if (ns <= 0 || !set.found) return;
    const int nrow = n + nq, rows_tile = std::min(nrow, exact_depth_rows_tile(bins)), tiles = (nrow + rows_tile - 1) / rows_tile;
    // a workgroup zeroes and flushes rows_tile * bins counters: it should have records enough to be worth them; and an LDS
    // counter is 32 bits wide: no workgroup takes 2^32 records
    const size_t groups = (set.found + 63) / 64, per_wg = (kDepthTallyThreads / 64) * kDepthGroupsPerWave;
    const size_t ranges = std::max(std::min<size_t>((groups + per_wg - 1) / per_wg, 256), (size_t)(set.found >> 31) + 1);
    const dim3 grid((unsigned)ranges, (unsigned)ns, (unsigned)tiles), block(kDepthTallyThreads);
    launch_full_lds<depth_tally_kernel>(grid, block, depth_tile_bytes((size_t)rows_tile, bins), st, set.mask, (unsigned long long)set.found,
                                        count_dev, n, nq, bins, rows_tile, table_dev, hist_dev, over_dev);
}

}  // namespace dd
