// dd_exact_screen.hip -- samples that are no leaves, screened against the ordered records of an exact universe.
//
// launch_exact_emit_order (dd_exact_sched.hip) leaves every distinct k-mer of the universe with its membership mask in
// ascending (hi, lo) order in HBM: a LocateSet.  Two kernels turn "sample s holds record r" into exact counts, and nothing
// but the counts leaves the device:
//
//   screen   screen_kernel: one thread per 64-token segment of a sample's token stream, one launch unit (gridDim.y) per
//            sample.  The token walk and the lookup in the ordered records are locate_kernel's (walk_segment and find_record
//            of dd_exact_walk.h).  An exact hit at record r sets bit r of the sample's SEEN bitmap (`found` bits in 32-bit
//            words, zeroed by the caller): the word is read with a plain load first and a no-return atomicOr is issued only
//            while the bit is still clear -- a read set at 30x coverage sets each bit once and then only reads; a stale read
//            costs one redundant atomic, never a wrong bit.  A miss is the normal case (a read set of another species).
//   tally    tally_kernel: the grid runs over (row, range of the records).  Row s < ns takes the records whose bit in
//            sample s's bitmap is set, row ns has no bitmap and takes every record: |G_i| and the size of every query class
//            come out of the same code.  A wave takes 64 consecutive records at a time, lane l the record 64 g + l (the
//            mask loads are contiguous, the seen words two per wave); a group without a set bit is skipped after that one
//            load.
//
// How the tally counts, and why: per-genome counters are PLANES from one-shot ballots, the form of AccPairwise
// (dd_exact_sched.hip) -- for every universe bit b, __ballot(bit b of the lane's mask) is the 64 records' column b, and lane
// b adds its popcount to a register: lane b owns genome b's sum.  That is one ballot, one count and one predicated add per
// (64 records, genome) and no state to flush mid-way, where 64 shift-and-adds per record would cost 128 VALU per record and
// a bit-sliced vertical counter (about 2 VALU per record) needs a flush every 2^planes records and 64 registers or an LDS
// transpose at each flush; the ballot form costs about 4 wave instructions per record-lane at n = 64 and is exact by
// construction.  The per-query counters take the same form: the pairs are staged in LDS, every lane tests its own record
// against pair q -- the (m & all) == all && (m & none) == 0 of dd_exact_select --, the ballot's popcount goes to lane q % 64,
// register q / 64.  There is no leader loop over a ballot anywhere: every ballot is consumed whole by one popcount.
// After the last group each thread adds its non-zero registers to the workgroup's counters in LDS once, and the workgroup
// issues one global atomicAdd per non-zero counter.  No atomic is issued per record.  Integer sums: the order of arrival
// does not change them, two calls return identical bytes.
#include <algorithm>
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void screen_kernel(const ExactGenome* __restrict__ samples, int k, LocateSet set,
                                                    uint32_t* seen, unsigned long long words) {
    const ExactGenome* u = samples + blockIdx.y;
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* mine = seen + (unsigned long long)blockIdx.y * words;
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long, int, uint64_t ah, uint64_t al, bool) {
        unsigned long long r;
        if (!find_record<WIDE>(set, ah, al, r)) return;
        uint32_t* word = mine + (r >> 5);   // (r < found: inside the row's ceil(found / 32) words)
        const uint32_t bit = 1u << (r & 31);
        if (!(*word & bit)) atomicOr(word, bit);
    });
}

constexpr int kTallyThreads = 256, kTallyQSlots = kScreenMaxQueries / 64;

__global__ __launch_bounds__(kTallyThreads) void tally_kernel(const uint64_t* __restrict__ mask, unsigned long long found,
                                                              const uint32_t* __restrict__ seen, unsigned long long words, int ns,
                                                              int n, int nq, const uint64_t* __restrict__ table,
                                                              unsigned long long* __restrict__ shared_out,
                                                              unsigned long long* __restrict__ match_out) {
    __shared__ uint64_t pair[2 * kScreenMaxQueries];
    __shared__ unsigned long long gen[64], hit[kScreenMaxQueries];
    const int row = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * nq; i += kTallyThreads) pair[i] = table[i];
    for (int i = threadIdx.x; i < nq; i += kTallyThreads) hit[i] = 0;
    if (threadIdx.x < 64) gen[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t* mine = row < ns ? seen + (unsigned long long)row * words : nullptr;
    const int lane = threadIdx.x & 63;
    unsigned long long gsum = 0, qsum[kTallyQSlots];
#pragma unroll
    for (int r = 0; r < kTallyQSlots; ++r) qsum[r] = 0;
    const unsigned long long groups = (found + 63) / 64, waves = (unsigned long long)gridDim.x * (kTallyThreads / 64);
    for (unsigned long long g = (unsigned long long)blockIdx.x * (kTallyThreads / 64) + (threadIdx.x >> 6); g < groups; g += waves) {
        const unsigned long long r = g * 64 + lane;
        bool has = r < found;
        if (has && mine) has = (mine[r >> 5] >> (r & 31)) & 1u;
        if (!__ballot(has)) continue;   // (the same in every lane of the wave)
        const uint64_t m = has ? mask[r] : 0ull;
        for (int b = 0; b < n; ++b) {
            const unsigned long long col = __ballot((m >> b) & 1ull);
            if (lane == b) gsum += (unsigned long long)__builtin_popcountll(col);
        }
#pragma unroll
        for (int slot = 0; slot < kTallyQSlots; ++slot) {
            if (slot * 64 >= nq) break;
            const int top = nq - slot * 64 < 64 ? nq - slot * 64 : 64;
            for (int l = 0; l < top; ++l) {
                const uint64_t al = pair[2 * (slot * 64 + l)], no = pair[2 * (slot * 64 + l) + 1];
                const unsigned long long col = __ballot(has && mask_matches(m, al, no));
                if (lane == l) qsum[slot] += (unsigned long long)__builtin_popcountll(col);
            }
        }
    }
    if (gsum) atomicAdd(&gen[lane], gsum);   // (lane b >= n never counted)
#pragma unroll
    for (int slot = 0; slot < kTallyQSlots; ++slot)
        if (qsum[slot]) atomicAdd(&hit[slot * 64 + lane], qsum[slot]);
    __syncthreads();
    if ((int)threadIdx.x < n && gen[threadIdx.x]) atomicAdd(&shared_out[(size_t)row * n + threadIdx.x], gen[threadIdx.x]);
    for (int q = threadIdx.x; q < nq; q += kTallyThreads)
        if (hit[q]) atomicAdd(&match_out[(size_t)row * nq + q], hit[q]);
}

}  // namespace

void launch_exact_screen(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set,
                         uint32_t* seen_dev, size_t words, hipStream_t st) {
    if (ns <= 0 || !max_segments || !set.found) return;
    launch_segment_walk((size_t)ns, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((screen_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, samples_dev, k, set, seen_dev,
                           (unsigned long long)words);
    });
}

void launch_exact_tally(const LocateSet& set, const uint32_t* seen_dev, size_t words, int ns, int n, int nq, const uint64_t* table_dev,
                        unsigned long long* shared_dev, unsigned long long* match_dev, hipStream_t st) {
    if (!set.found) return;
    // a workgroup flushes up to n + nq counters: few enough of them per row that the flushes stay small next to the records
    const size_t groups = (set.found + 63) / 64, per_wg = kTallyThreads / 64;
    const dim3 grid((unsigned)std::min<size_t>((groups + per_wg - 1) / per_wg, 256), (unsigned)(ns + 1)), block(kTallyThreads);
    hipLaunchKernelGGL(tally_kernel, grid, block, 0, st, set.mask, set.found, seen_dev, (unsigned long long)words, ns, n, nq, table_dev,
                       shared_dev, match_dev);
}

}  // namespace dd
