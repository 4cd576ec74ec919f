// dd_exact_gather.hip -- samples that are no leaves, EXPLAINED by the genomes of an exact universe one by one: the greedy
// minimum set cover over the records a sample holds (what `sourmash gather` made standard), exact and on the device.
//
// dd_exact_screen.hip and dd_exact_depth.hip count every genome against the whole sample, independently.  Here the genomes
// are picked in turn: the one that holds most of the sample's records that no earlier pick holds, then the next over what is
// left.  Behind the ordered records (a LocateSet: one 64-bit membership mask per record) and depth_kernel's counters (one
// 32-bit depth per (sample, record), dd_exact_depth.hip, used as it is), a walk is a loop of two launches per step over the
// samples of a round, with a small state per sample -- {taken: the picks so far as a mask, last: the pick whose depth is
// still open} -- and no host round trip inside it:
//
//   gather   gather_kernel: the grid runs over (range of the records, sample of the round).  A wave takes 64 consecutive
//            records, lane l the record 64 g + l, and loads their counters; a group whose counters are all zero is skipped
//            after that one load and one ballot.  A record is LIVE when the sample holds it (counter > 0) and its mask meets
//            `taken` nowhere.  The live records whose mask has bit `last` are the previous pick's own: they add their counter
//            to a 64-bit register sum -- that closes the previous step's depth -- and take no part in the ballots, since the
//            fold of `last` into `taken` kills them.  The other live records go through one __ballot per CANDIDATE bit b, a
//            bit of the universe outside taken | 1 << last: lane b adds the ballot's popcount to its register, tally_kernel's
//            form (dd_exact_screen.hip), and the loop over the candidates shrinks as the walk goes on.  On the first pass
//            (nothing picked) the same loads also count the sample's held records and the sum of their depths.  After the
//            last group each thread adds its non-zero registers to the workgroup's counters in LDS once, and the workgroup
//            issues one global atomicAdd per non-zero counter.  No atomic is issued per record.  Integer sums: the order of
//            arrival does not change them, two calls return identical bytes.  The workgroups of a sample whose walk has
//            stopped return after reading the state.
//   pick     gather_pick_kernel: one wave per sample of the round.  It writes the closed step's depth from the depth sum and
//            clears the sum, folds `last` into `taken`, takes the argmax of the 64 step counters (a butterfly over the wave,
//            the lowest index on a tie), applies the stop rule -- fewer than min_hits records, or no step left --, writes
//            pick / unique of the step, copies the counters to `shared` on step 0 (nothing is taken yet: they are screen's
//            shared[s][b]) and zeroes them for the next pass.
//
// The state's `last` is stored plus one, so that the round's one memset leaves a fresh walk in it.
#include <algorithm>
#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kGatherThreads = 256;
constexpr size_t kGatherGroupsPerWave = 16;   // record groups a wave should have before another workgroup is worth its flush
constexpr unsigned kGatherMaxRanges = 2048;   // 8 workgroups of 4 waves per CU: the rest is the grid-stride loop

__global__ __launch_bounds__(kGatherThreads) void gather_kernel(const uint64_t* __restrict__ mask, unsigned long long found,
                                                                const uint32_t* __restrict__ count, int n,
                                                                const GatherState* __restrict__ state,
                                                                unsigned long long* __restrict__ step_out,
                                                                unsigned long long* __restrict__ sums_out) {
    __shared__ unsigned long long gen[64], sums[kGatherSums];
    const GatherState st = state[blockIdx.y];
    if (st.last1 == kGatherDone) return;   // (the same in every thread of the workgroup)
    const int last = st.last1 - 1;         // -1: the first pass
    const bool first = last < 0;
    if (threadIdx.x < 64) gen[threadIdx.x] = 0;
    if (threadIdx.x < kGatherSums) sums[threadIdx.x] = 0;
    __syncthreads();
    // wave-uniform, in scalar registers: the picks so far, the open pick's bit, the candidates of this pass
    const uint64_t taken = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)st.taken) |
                           (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(st.taken >> 32)) << 32;
    const uint64_t open = first ? 0ull : 1ull << last;
    const uint64_t cands = (n < 64 ? (1ull << n) - 1 : ~0ull) & ~(taken | open);
    const uint32_t* mine = count + (unsigned long long)blockIdx.y * found;
    const int lane = threadIdx.x & 63;
    unsigned long long usum = 0, dsum = 0, held_n = 0, held_d = 0;
    const unsigned long long groups = (found + 63) / 64, waves = (unsigned long long)gridDim.x * (kGatherThreads / 64);
    for (unsigned long long g = (unsigned long long)blockIdx.x * (kGatherThreads / 64) + (threadIdx.x >> 6); g < groups; g += waves) {
        const unsigned long long r = g * 64 + lane;
        const uint32_t c = r < found ? mine[r] : 0u;
        const bool held = c != 0;
        if (!__ballot(held)) continue;   // (the same in every lane of the wave)
        const uint64_t m = held ? mask[r] : 0ull;
        if (first && held) held_n += 1, held_d += c;
        const bool live = held && !(m & taken);
        const bool closing = live && (m & open);
        if (closing) dsum += c;
        const uint64_t mc = live && !closing ? m : 0ull;   // (a record's mask is never 0)
        if (!__ballot(mc != 0)) continue;
        for (uint64_t todo = cands; todo; todo &= todo - 1) {
            const int b = __builtin_ctzll(todo);
            const unsigned long long col = __ballot((mc >> b) & 1ull);
            if (lane == b) usum += (unsigned long long)__builtin_popcountll(col);
        }
    }
    if (usum) atomicAdd(&gen[lane], usum);   // (lane b outside the candidates never counted)
    if (dsum) atomicAdd(&sums[kGatherOpenDepth], dsum);
    if (held_n) atomicAdd(&sums[kGatherHeld], held_n), atomicAdd(&sums[kGatherHeldDepth], held_d);
    __syncthreads();
    if (threadIdx.x < 64 && gen[threadIdx.x]) atomicAdd(&step_out[(size_t)blockIdx.y * 64 + threadIdx.x], gen[threadIdx.x]);
    if (threadIdx.x < kGatherSums && sums[threadIdx.x]) atomicAdd(&sums_out[(size_t)blockIdx.y * kGatherSums + threadIdx.x], sums[threadIdx.x]);
}

__global__ __launch_bounds__(64) void gather_pick_kernel(GatherState* __restrict__ state, unsigned long long* __restrict__ step,
                                                         unsigned long long* __restrict__ sums, int n, int t, int steps, uint32_t min_hits,
                                                         int32_t* __restrict__ pick, unsigned long long* __restrict__ unique,
                                                         unsigned long long* __restrict__ depth, unsigned long long* __restrict__ shared) {
    const size_t s = blockIdx.x;
    const int lane = threadIdx.x;
    GatherState st = state[s];
    const unsigned long long v = step[s * 64 + lane];
    step[s * 64 + lane] = 0;
    const int last = st.last1 - 1;
    if (last >= 0) {   // (so t >= 1) step t - 1 picked `last`: the pass in front of this launch summed its records' depths
        if (lane == 0) depth[s * steps + (t - 1)] = sums[s * kGatherSums + kGatherOpenDepth], sums[s * kGatherSums + kGatherOpenDepth] = 0;
        st.taken |= 1ull << last;
    }
    if (t == 0 && lane < n) shared[s * n + lane] = v;
    unsigned long long best = v;
    int at = lane;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d);
        const int where = __shfl_xor(at, d);
        if (other > best || (other == best && where < at)) best = other, at = where;
    }
    // (a walk that has stopped has all-zero counters, and min_hits >= 1: it stays stopped)
    const bool go = st.last1 != kGatherDone && t < steps && best >= min_hits;
    if (lane == 0) {
        if (t < steps) {
            pick[s * steps + t] = go ? at : -1;
            if (go) unique[s * steps + t] = best;
        }
        st.last1 = go ? at + 1 : kGatherDone;
        state[s] = st;
    }
}

}  // namespace

void launch_exact_gather(const LocateSet& set, const uint32_t* count_dev, int ns, int n, const GatherState* state_dev,
                         unsigned long long* step_dev, unsigned long long* sums_dev, hipStream_t st) {
    if (ns <= 0 || !set.found) return;
    // a workgroup zeroes and flushes 64 + kGatherSums counters: it should have records enough to be worth them
    const size_t groups = (set.found + 63) / 64, per_wg = (kGatherThreads / 64) * kGatherGroupsPerWave;
    const dim3 grid((unsigned)std::min<size_t>((groups + per_wg - 1) / per_wg, kGatherMaxRanges), (unsigned)ns), block(kGatherThreads);
    hipLaunchKernelGGL(gather_kernel, grid, block, 0, st, set.mask, (unsigned long long)set.found, count_dev, n, state_dev, step_dev, sums_dev);
}

void launch_exact_gather_pick(int ns, int n, int t, int steps, uint32_t min_hits, GatherState* state_dev, unsigned long long* step_dev,
                              unsigned long long* sums_dev, int32_t* pick_dev, unsigned long long* unique_dev, unsigned long long* depth_dev,
                              unsigned long long* shared_dev, hipStream_t st) {
    if (ns <= 0) return;
    hipLaunchKernelGGL(gather_pick_kernel, dim3((unsigned)ns), dim3(64), 0, st, state_dev, step_dev, sums_dev, n, t, steps, min_hits, pick_dev,
                       unique_dev, depth_dev, shared_dev);
}

}  // namespace dd
