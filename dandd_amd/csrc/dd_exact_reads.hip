// dd_exact_reads.hip -- samples that are no leaves, called record by record with the genomes of an exact universe.
//
// dd_exact_paint.hip cuts a sample's token stream into fixed windows; a read set is no such thing: a window of 4096 tokens
// holds 27 reads of 150 bases, one of 64 tokens the ends of two.  Here the rows are the caller's: sample s owns the rows
// off[s] .. off[s+1]-1, row r covers the tokens start[r] .. start[r+1]-1 (the sample's last row runs to ntok, the tokens in
// front of its first border belong to no row), and behind the same ordered records (a LocateSet) two kernels leave what a
// user asks of a read set: which genome each row belongs to, and how many rows of a sample go to each genome.
//
//   reads    reads_kernel: paint_kernel's shape, walk, lookup and bit-sliced per-genome counter -- one thread per 64-token
//            segment, gridDim.y = sample, kPaintPlanes 64-bit planes that take set.mask[r] by a ripple carry -- with rows
//            from borders.  A k-mer counts in the row that holds its END token (dd_exact_locate's and paint's convention);
//            where the borders are record starts it lies whole inside that record, K0 puts a BREAK in front of every record.
//   vote     vote_kernel: one thread per row reads the row's n + 2 counters once and writes its call (best and second
//            genome, the sets of the tied and of the consistent genomes); the call's class goes to a histogram of n + 3 bins
//            in LDS -- a workgroup serves one sample, gridDim.y again -- and the workgroup issues one no-return 64-bit
//            atomicAdd per non-zero bin (tally_kernel's end).  No floating point anywhere.
//
// The border walk.  A thread finds the row of its first token once: an upper bound of seg * 64 in its sample's borders,
// ceil(log2 rows) dependent 8-byte reads, the first levels of which every thread shares.  It keeps the NEXT border in a
// register; the callback of the walk, which runs at k-mer ends only, compares the token with it, and where the token has
// reached it the thread flushes its counters to the row it leaves, clears them and steps over the borders up to the token
// (a loop: empty records make runs of one-token rows; the borders ascend strictly, so a segment holds 64 of them at the
// most).  Behind the walk it flushes once more.
//
// Seven planes still suffice: the planes are cleared at every flush and a thread's whole run is 64 tokens, so between two
// flushes it ends at most 64 = 1000000b k-mers -- paint_kernel's bound, which borders can only lower.
//
// How the counters reach the row:
//   the wave in one row       where the first and the last live token of a wave lie in the same row (a contig, a
//                             chromosome: every wave but those at record borders) no lane ever meets a border.  That is
//                             known before the walk, from two searches that are the same in every lane, and the wave takes
//                             paint's ballot path: one __ballot per plane and genome, lane i adds its popcount, at most
//                             n + 2 no-return atomicAdds per wave.  A wave that lies in front of the first border returns.
//   otherwise                 every live thread adds its non-zero counts to the row it is in, at each border and at the end
//                             (paint's third path).  Reads of 150 bases: 2-3 segments to a row, 2-3 flushes of at most
//                             n + 2 atomics per row.
// Integer sums: the order of arrival does not change them, two calls return identical bytes.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

// the borders of b[0 .. len) that are <= tok: the row of the token is that number less one (none: it lies in front of them)
DD_D unsigned long long borders_upto(const unsigned long long* __restrict__ b, unsigned long long len, unsigned long long tok) {
    unsigned long long first = 0;
    while (len) {
        const unsigned long long half = len >> 1;
        if (b[first + half] <= tok) first += half + 1, len -= half + 1;
        else len = half;
    }
    return first;
}

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void reads_kernel(const ExactGenome* __restrict__ samples, int k, LocateSet set, int n,
                                                   const unsigned long long* __restrict__ off,
                                                   const unsigned long long* __restrict__ start, uint32_t* counts) {
    const ExactGenome* u = samples + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long first = seg - (unsigned)lane;   // the wave's first segment: live if any of them is
    if (first * kSegTokens >= ntok) return;
    const unsigned long long row0 = off[blockIdx.y], nrow = off[blockIdx.y + 1] - row0;
    if (!nrow) return;   // (a sample without a row)
    const unsigned long long* border = start + row0;
    const unsigned long long ncol = (unsigned long long)n + 2;
    uint32_t* rows = counts + row0 * ncol;
    const bool live = seg * kSegTokens < ntok;
    // the same in every lane: the borders at or in front of the wave's first token and of its last live one
    const unsigned long long end = first * kSegTokens + (64 * kSegTokens - 1), lasttok = end < ntok - 1 ? end : ntok - 1;
    const unsigned long long upto_first = borders_upto(border, nrow, first * kSegTokens);
    const bool one_row = upto_first == borders_upto(border, nrow, lasttok);
    if (one_row && !upto_first) return;   // the whole wave in front of the first border
    if (!one_row && !live) return;
    // `have` borders lie at or in front of the thread's token: it is in row have - 1 (have = 0: in no row yet), and `next`
    // is the border that ends that row
    unsigned long long have = one_row ? upto_first : borders_upto(border, nrow, seg * kSegTokens);
    unsigned long long next = have < nrow ? border[have] : ~0ull;
    PlaneCounter pc;
    pc.clear();
    uint32_t valid = 0, inpan = 0;
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long sidx, int t, uint64_t ah, uint64_t al, bool) {
        const unsigned long long tok = sidx * kSegTokens + (unsigned)t;
        if (tok >= next) {   // (never in a wave that lies in one row)
            if (have && valid) pc.flush(rows + (have - 1) * ncol, n, valid, inpan);   // (have <= nrow: one of the sample's rows)
            valid = 0, inpan = 0, pc.clear();
            do {
                ++have;
                next = have < nrow ? border[have] : ~0ull;
            } while (tok >= next);
        }
        ++valid;
        unsigned long long r;
        if (find_record<WIDE>(set, ah, al, r)) ++inpan, pc.add(set.mask[r]);
    });
    if (one_row) pc.flush_wave(rows + (upto_first - 1) * ncol, n, lane, valid, inpan);   // (the same in every lane)
    else if (have && valid) pc.flush(rows + (have - 1) * ncol, n, valid, inpan);
}

constexpr int kVoteThreads = 256;
constexpr uint32_t kNoGenome = 0xFFFFFFFFu;

// One thread per row.  best: the largest column, a tie to the lower index (a later column takes over only where it is
// larger); second: the largest non-zero column among the others, a tie to the lower index -- a best that is taken over
// becomes the second (it is no smaller than the second so far, and where equal it is the earlier one).
__global__ __launch_bounds__(kVoteThreads) void vote_kernel(const uint32_t* __restrict__ counts, const unsigned long long* __restrict__ off,
                                                            int n, uint32_t min_hits, uint32_t* __restrict__ calls,
                                                            uint64_t* __restrict__ sets, unsigned long long* __restrict__ tally) {
    __shared__ uint32_t bin[kReadsClasses];
    const int nbin = n + 3;
    for (int i = threadIdx.x; i < nbin; i += kVoteThreads) bin[i] = 0;
    __syncthreads();
    const unsigned long long row0 = off[blockIdx.y], nrow = off[blockIdx.y + 1] - row0;
    const unsigned long long r = (unsigned long long)blockIdx.x * kVoteThreads + threadIdx.x;
    if (r < nrow) {
        const uint32_t* row = counts + (row0 + r) * ((unsigned long long)n + 2);
        const uint32_t valid = row[0], hit = row[1];
        uint32_t best = kNoGenome, best_count = 0, second = kNoGenome, second_count = 0;
        uint64_t ties = 0, full = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t v = row[2 + i];
            if (hit && v == hit) full |= 1ull << i;
            if (v > best_count) {
                second = best, second_count = best_count;
                best = (uint32_t)i, best_count = v;
                ties = 1ull << i;
            } else if (v) {
                if (v == best_count) ties |= 1ull << i;
                if (v > second_count) second = (uint32_t)i, second_count = v;
            }
        }
        if (calls) {
            uint32_t* c = calls + (row0 + r) * 6;
            c[0] = valid, c[1] = hit, c[2] = best, c[3] = best_count, c[4] = second, c[5] = second_count;
        }
        if (sets) {
            uint64_t* s = sets + (row0 + r) * 2;
            s[0] = ties, s[1] = full;
        }
        // the class: no valid k-mer | unclassified | unique to `best` | ambiguous
        const int cls = !valid ? n + 2 : best_count < min_hits ? n + 1 : (ties & (ties - 1)) ? n : (int)best;
        atomicAdd(&bin[cls], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbin; i += kVoteThreads)
        if (bin[i]) atomicAdd(&tally[(unsigned long long)blockIdx.y * nbin + i], (unsigned long long)bin[i]);
}

}  // namespace

void launch_exact_reads(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set, int n,
                        const unsigned long long* off_dev, const unsigned long long* start_dev, uint32_t* counts_dev, hipStream_t st) {
    if (ns <= 0 || !max_segments) return;
    launch_segment_walk((size_t)ns, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((reads_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, samples_dev, k, set, n, off_dev,
                           start_dev, counts_dev);
    });
}

void launch_exact_vote(const uint32_t* counts_dev, const unsigned long long* off_dev, int ns, size_t max_rows, int n, uint32_t min_hits,
                       uint32_t* calls_dev, uint64_t* sets_dev, unsigned long long* tally_dev, hipStream_t st) {
    if (ns <= 0 || !max_rows) return;
    const dim3 grid((unsigned)((max_rows + kVoteThreads - 1) / kVoteThreads), (unsigned)ns), block(kVoteThreads);
    hipLaunchKernelGGL(vote_kernel, grid, block, 0, st, counts_dev, off_dev, n, min_hits, calls_dev, sets_dev, tally_dev);
}

}  // namespace dd
