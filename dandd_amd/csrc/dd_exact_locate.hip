// dd_exact_locate.hip -- where the selected k-mers lie: every position of a genome looked up in the emitted set.
//
// The emission leaves the distinct k-mers whose membership mask matches a query in HBM (emit_kernel of dd_exact_sched.hip:
// lo | hi | mask, in the order the chunks of the sort finished, over all passes).  Two steps turn that set into positions,
// and neither leaves the device:
//
//   order    launch_exact_emit_order (dd_exact_sched.hip, shared with dd_exact_select_kmers): the records in ascending
//            (hi, lo) order.  The exact workspace is free by then and holds the sort's other halves and temp.
//   locate   locate_kernel: one thread per 64-token segment of a painted genome, the token walk of kmer_extract_kernel
//            (walk_segment of dd_exact_walk.h: the segment in front warms the windows up, run >= k, canonical per the
//            context, keys under the key masks).  Every k-mer is looked up in the ordered records (find_record, there).  A
//            k-mer that matches no query is not in the set: a miss is the normal case.  On an exact hit the record's mask is
//            tested against the up to kLocateJobs (all, none) pairs of the launch unit (staged in LDS), one 64-bit word of
//            hit bits per job is kept in registers, and the thread -- the only owner of its segment's word -- writes them
//            with plain stores: no atomics.  The padding behind ntok is BREAK tokens, so bits at or beyond ntok stay 0.
//
// Why a search and not a join by sorting: the positions of a genome would have to be sorted by key (the universe's sort
// again, per genome) and scattered back; the set is small next to the positions (markers are a few per cent of a genome)
// and its top levels stay in L2.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

template <bool CANON, bool WIDE>
__global__ __launch_bounds__(256) void locate_kernel(const LocateUnit* __restrict__ units, int k, LocateSet set,
                                                    uint64_t* __restrict__ hits) {
    __shared__ uint64_t sall[kLocateJobs], snone[kLocateJobs];
    __shared__ unsigned long long sout[kLocateJobs];
    const LocateUnit* u = units + blockIdx.y;
    const int nj = u->nj;
    if (threadIdx.x < kLocateJobs) {
        sall[threadIdx.x] = u->all[threadIdx.x];
        snone[threadIdx.x] = u->none[threadIdx.x];
        sout[threadIdx.x] = u->out[threadIdx.x];
    }
    __syncthreads();
    const unsigned long long ntok = *u->ntok;
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (seg * kSegTokens >= ntok) return;
    uint64_t word[kLocateJobs];
#pragma unroll
    for (int j = 0; j < kLocateJobs; ++j) word[j] = 0;
    walk_segment<CANON, false>(u->codes, u->bad, ntok, seg, k, [&](unsigned long long, int t, uint64_t ah, uint64_t al, bool) {
        unsigned long long r;
        if (!find_record<WIDE>(set, ah, al, r)) return;
        const uint64_t m = set.mask[r];
#pragma unroll
        for (int j = 0; j < kLocateJobs; ++j) {
            const bool hit = (j < nj) & mask_matches(m, sall[j], snone[j]);   // (&, not &&: a branch per job cost 7 % at k = 21)
            word[j] |= (uint64_t)hit << t;
        }
    });
#pragma unroll
    for (int j = 0; j < kLocateJobs; ++j)
        if (j < nj) hits[sout[j] + seg] = word[j];
}

}  // namespace

void launch_exact_locate(const LocateUnit* units_dev, int nunits, size_t max_segments, int k, int canonical, const LocateSet& set,
                         uint64_t* hits_dev, hipStream_t st) {
    if (nunits <= 0 || !max_segments || !set.found) return;
    launch_segment_walk((size_t)nunits, max_segments, canonical, k, [&](dim3 grid, dim3 block, auto cn, auto wd) {
        hipLaunchKernelGGL((locate_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, units_dev, k, set, hits_dev);
    });
}

}  // namespace dd
