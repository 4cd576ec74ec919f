// dd_exact_locate.hip -- where the selected k-mers lie: every position of a genome looked up in the emitted set.
//
// The emission leaves the distinct k-mers whose membership mask matches a query in HBM (emit_kernel of dd_exact_sched.hip:
// lo | hi | mask, in the order the chunks of the sort finished, over all passes).  Two steps turn that set into positions,
// and neither leaves the device:
//
//   order    launch_exact_emit_order (dd_exact_sched.hip, shared with dd_exact_select_kmers): the records in ascending
//            (hi, lo) order.  The exact workspace is free by then and holds the sort's other halves and temp.
//   locate   locate_kernel: one thread per 64-token segment of a painted genome, the token walk of kmer_extract_kernel
//            (dd_exact.hip: the segment in front warms the windows up, run >= k, canonical per the context).  At every
//            valid window the key is formed under mlo / mhi and looked up with a lower_bound on (hi, lo): ceil(log2 found)
//            dependent 8- or 16-byte reads, the first levels of which every thread shares (L2).  A k-mer that matches no
//            query is not in the set: a miss is the normal case.  On an exact hit the record's mask is tested against the
//            up to kLocateJobs (all, none) pairs of the launch unit (staged in LDS), one 64-bit word of hit bits per job
//            is kept in registers, and the thread -- the only owner of its segment's word -- writes them with plain stores:
//            no atomics.  The padding behind ntok is BREAK tokens, so bits at or beyond ntok stay 0.
//
// Why a search and not a join by sorting: the positions of a genome would have to be sorted by key (the universe's sort
// again, per genome) and scattered back; the set is small next to the positions (markers are a few per cent of a genome)
// and its top levels stay in L2.
// (The walk is a copy of kmer_extract_kernel's, not shared code: that kernel keeps every lane in the token loop for its
// wave-level append, so a common walk would have to be threaded through its hot loop.)
#include "dd_common.h"
#include "dd_kernels.h"

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
    const uint4* codes4 = reinterpret_cast<const uint4*>(u->codes);
    const uint2* bad2 = reinterpret_cast<const uint2*>(u->bad);
    uint64_t word[kLocateJobs];
#pragma unroll
    for (int j = 0; j < kLocateJobs; ++j) word[j] = 0;
    uint64_t fh = 0, fl = 0, rh = 0, rl = 0;
    int run = 0;
    const uint64_t mlo = (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const uint64_t mhi = (k <= 32) ? 0ull : ((k == 64) ? ~0ull : ((1ull << (2 * k - 64)) - 1ull));
    const int s = 128 - 2 * k;  // right shift that aligns the reverse-complement window
    for (int part = (seg > 0 ? 0 : 1); part < 2; ++part) {
        const unsigned long long sidx = seg - 1 + part;
        const uint4 c4 = codes4[sidx];
        const uint2 b2 = bad2[sidx];
        const uint32_t cw[4] = {c4.x, c4.y, c4.z, c4.w};
        const uint64_t bw = ((uint64_t)b2.y << 32) | b2.x;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll 1
        for (int i = 0; i < 16; ++i) {
            const int t = w * 16 + i;
            const uint32_t c = (cw[w] >> (2 * i)) & 3u;
            run = ((bw >> t) & 1ull) ? 0 : run + 1;
            fh = (fh << 2) | (fl >> 62);
            fl = (fl << 2) | c;
            rl = (rl >> 2) | (rh << 62);
            rh = (rh >> 2) | ((uint64_t)(3u - c) << 62);
            if (part == 0 || run < k) continue;
            uint64_t ah = fh & mhi, al = fl & mlo;
            if (CANON) {
                uint64_t bh, bl;
                if (s >= 64) {
                    bh = 0;
                    bl = rh >> (s - 64);
                } else if (s == 0) {
                    bh = rh;
                    bl = rl;
                } else {
                    bh = rh >> s;
                    bl = (rl >> s) | (rh << (64 - s));
                }
                if (bh < ah || (bh == ah && bl < al)) {
                    ah = bh;
                    al = bl;
                }
            }
            // lower_bound on (hi, lo) over the ordered records
            unsigned long long first = 0, len = set.found;
            while (len) {
                const unsigned long long half = len >> 1, mid = first + half;
                const uint64_t l = set.lo[mid];
                bool less = l < al;
                if (WIDE) {
                    const uint64_t h = set.hi[mid];
                    less = h < ah || (h == ah && less);
                }
                if (less) first = mid + 1, len -= half + 1;
                else len = half;
            }
            if (first >= set.found || set.lo[first] != al) continue;
            if (WIDE && set.hi[first] != ah) continue;
            const uint64_t m = set.mask[first];
#pragma unroll
            for (int j = 0; j < kLocateJobs; ++j) {
                const bool hit = j < nj && (m & sall[j]) == sall[j] && (m & snone[j]) == 0;
                word[j] |= (uint64_t)hit << t;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kLocateJobs; ++j)
        if (j < nj) hits[sout[j] + seg] = word[j];
}

}  // namespace

void launch_exact_locate(const LocateUnit* units_dev, int nunits, size_t max_segments, int k, int canonical, const LocateSet& set,
                         uint64_t* hits_dev, hipStream_t st) {
    if (nunits <= 0 || !max_segments || !set.found) return;
    const dim3 grid((unsigned)((max_segments + 255) / 256), (unsigned)nunits), block(256);
    dispatch_bool(canonical != 0, [&](auto cn) {
        dispatch_bool(k > 32, [&](auto wd) {
            hipLaunchKernelGGL((locate_kernel<decltype(cn)::value, decltype(wd)::value>), grid, block, 0, st, units_dev, k, set, hits_dev);
        });
    });
}

}  // namespace dd
