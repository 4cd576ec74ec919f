// dd_sweep.hip -- K1: fused k-sweep HyperLogLog sketch over the 2-bit token stream.
//
// Replaces  parallel -j 95% ' dashing sketch -k{} -S <p> --prefix <dir> <fasta> ' ::: kmin..kmax
// (/root/reference/lib/huffman_dandd.py:214-218, /root/reference/lib/sketch_classes.py:351-366):
// instead of one process per k, each re-reading and re-parsing the FASTA, one launch walks the
// token stream once per k-group, with the group's register arrays resident in LDS.
//
// Work decomposition
//   job (one workgroup) = (genome, k-group, range of tiles); tile = blockDim.x segments of 64
//   tokens; a thread owns one segment per tile: it loads the segment's 16 B of codes + 8 B of
//   BREAK bits and the previous segment's (the halo that primes the rolling windows), then for
//   each token updates one shared forward / reverse-complement window and, for every k of the
//   group, masks/shifts the k-mer out of the windows, canonicalises, hashes (Wang 64), and
//   raises LDS register  reg[k][h >> (64-p)]  to  rho(h).
//   The LDS registers are byte-max-merged into the genome's [K][m] slab in HBM at job end.
//
// Bound: integer VALU issue.  Measured issue costs on gfx950 (scripts/ubench.hip, 4 waves/SIMD,
// 2.34 GHz): v_xor/and/or/not/mov/add/sub/lshrrev_b32 ~2.5 cycles per wave64 instruction;
// everything else used here (v_lshlrev_b32, v_alignbit, v_mul_lo_u32, v_ffbh, v_cmp, v_cndmask and
// every 64-bit op: v_lshrrev_b64, v_lshl_add_u64, v_mad_u64_u32, v_cmp_lt_u64) ~4.2 cycles.  A 64-bit
// instruction therefore costs the same as one 32-bit shift, so the hash (dd_k1.h) is written in 64-bit
// instructions -- 18 of them, 16 where the key has one word -- and 32-bit work is steered to the cheap class.
// Per token of a BREAK-free wave the canonical kernels issue (token-loop head + one k-pair body up to the "no register
// rises" branch, profiles/k1_hash17.txt): 2 + 47 for k 10..16, 4 + 55 for k 17..32, 6 + 73 for k 33..48.
// HBM traffic is 3 bits per token per k-group.  No MFMA: this is hashing, not a contraction.
//
// Rows of k = 10..14 that have reached sketch(U_k), the row of all k-mers (universe_kernel), are flagged at the merge and left
// out by the jobs that start later (dd_kernels.h, saturation; profiles/k1_saturation.txt): outside the token loop.
//
// This file: the registers-in-LDS family (log2m <= 16: sweep_kernel) and the set classes (bitmap_kernel, bigmap_kernel and their
// finish kernels).  The record path of log2m >= 17 is dd_scatter.hip; what both share (hash, windows, tile input, token walk,
// launch helpers) is dd_k1.h.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_k1.h"

namespace dd {
namespace {

// every k of the group for the token just pushed; reached by whole waves (the raise queue's count is wave-uniform)
template <int KC, bool CANON, bool CHECK, typename Win>
DD_D void sweep_token(const Win& win, int run, int kfirst, int nk, int p, RaiseQueue& s) {
    // The loop counter stays wave-uniform in both variants (k-dependent masks and shifts are then
    // scalar); in the CHECK variant lanes whose run is too short for k hash their window all the same and are
    // left out of the update (ok), and the ks no lane of the wave has a window for are skipped.
    constexpr bool QUEUE = KC != 0;
    // nk as an opaque scalar copy: the odd-k test `j < nk` behind the pair loop then stays an s_cmp.  Without it the
    // compiler hoists the loop-invariant `nk < 2` out of the caller's token loop as a lane mask and re-makes it per token
    // with a v_cndmask_b32 + v_cmp_ne_u32 pair (profiles/k1_sliced_windows.txt, section 3).
    asm volatile("" : "+s"(nk));
    int j = 0;
#pragma unroll 1
    for (; j + 1 < nk; j += 2) {
        const int k = kfirst + j;
        const bool ok0 = !CHECK || run >= k, ok1 = !CHECK || run > k;
        const unsigned long long okm0 = CHECK ? __builtin_amdgcn_ballot_w64(run >= k) : ~0ull, okm1 = CHECK ? __builtin_amdgcn_ballot_w64(run > k) : ~0ull;
        if (CHECK && !okm0) return;
        sweep_update2<QUEUE, CHECK>(s, (uint32_t)j, win.template hash<CANON>(k), okm0, ok0,
                                    (uint32_t)j + 1u, win.template hash<CANON>(k + 1), okm1, ok1, p);
    }
    if (j < nk) {
        const int k = kfirst + j;
        const unsigned long long okm = CHECK ? __builtin_amdgcn_ballot_w64(run >= k) : ~0ull;
        if (!CHECK || okm) sweep_update<QUEUE, CHECK>(s, (uint32_t)j, win.template hash<CANON>(k), okm, !CHECK || run >= k, p);
    }
}

// The registers of the job's k-group live in LDS (2^p * nk bytes <= 160 KiB): log2m <= 16.
template <int KC, bool CANON>
__global__ __launch_bounds__(1024) void sweep_kernel(const SweepGenome* __restrict__ genomes,
                                                    const SweepJob* __restrict__ jobs, int p, uint32_t queue_off,
                                                    const uint8_t* __restrict__ universe, int universe_last_k) {
    lds_starts_at_zero();
    const SweepJob job = jobs[blockIdx.x];
    const SweepGenome g = genomes[job.genome];
    int nk = job.nk, kfirst = job.kfirst, krow = job.krow;
    const uint32_t m = 1u << p;

    // Saturation (dd_kernels.h; the 32-bit class only: universe rows exist for k <= kSatMaxK): the first nsat rows of the group
    // have a universe row.  Those of them that earlier jobs found equal to it are final: a flagged PREFIX of the group is left
    // out (smaller k saturates first, and the ks that remain stay consecutive, the LDS layout compact).
    // ONE thread reads the flags for the workgroup (bitmap_kernel: waves that read at different times would disagree), and
    // the count goes through a word of g_lds -- this kernel has no static LDS (lds_starts_at_zero) --, with a barrier on
    // each side before the warm start overwrites it.  A flag raised after this point changes nothing for the job.
    int nsat = 0;
    if constexpr (KC == 0) {
        if (g.sat && kfirst <= universe_last_k) nsat = min(nk, universe_last_k - kfirst + 1);
        if (nsat) {
            uint32_t* const word = reinterpret_cast<uint32_t*>(g_lds);
            if (threadIdx.x == 0) {
                uint32_t d = 0;
                while (d < (uint32_t)nsat && load4_fresh(g.sat + krow + d)) ++d;
                *word = d;
            }
            __syncthreads();
            const int d = __builtin_amdgcn_readfirstlane((int)*word);
            __syncthreads();
            kfirst += d, nk -= d, krow += d, nsat -= d;
            if (nk == 0) return;  // (before anything is loaded)
        }
    }
    const unsigned long long ntok = gload8u(g.ntok);
    uint8_t* const slab = g.regs + ((size_t)krow << p);

    // (the loads of tile t+1 are issued before tile t is processed, and those of the first tile before the warm start below)
    TileIn next;
    fetch_tile(g, job, ntok, job.tile_begin, next);

    {
        // Warm start: begin from whatever earlier jobs have already merged into the slab.  Any
        // (possibly stale) snapshot is a valid lower bound of the final registers, and a warm
        // array makes the "register rises" path rare: after T tokens have been absorbed only
        // ~m/T of the updates still raise a register.
        // The snapshot is read with agent-scope loads: other XCDs merge into the slab with
        // memory-side atomics, which a plain load served by THIS XCD's L2 would not see (it kept
        // returning the zeroed lines: every flush then CAS-ed every word and jobs started cold).
        uint4* z = reinterpret_cast<uint4*>(g_lds);
        const uint32_t n16 = (uint32_t)nk * (m >> 4);
        for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) z[i] = load16_fresh(slab + (size_t)i * 16);
    }
    __syncthreads();

    const int kmaxg = kfirst + nk - 1;
    // (queue_off: where the plan put the workgroup's raise queues, 0 = it had no room for them)
    RaiseQueue s;
    s.base = queue_off + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (kRaiseQueueRecords * 4u);
    s.dense = (KC != 0 && queue_off) ? kRaiseDense : 0u;
    s.waiting = 0;

    for (unsigned tile = job.tile_begin; tile < job.tile_end; ++tile) {
        const TileIn cur = next;
        fetch_tile(g, job, ntok, tile + 1, next);
        // Lanes beyond the stream stay in the loop as all-BREAK segments while any lane of their wave has tokens: the
        // raise queue is the wave's, and every append and flush must be reached by the whole wave.
        if (!__any(cur.live)) continue;
        SweepWindows<KC> win;
        walk_segment(cur, win, [&](auto clean, int run) {
            if constexpr (decltype(clean)::value) {
                sweep_token<KC, CANON, false>(win, 0, kfirst, nk, p, s);
            } else {
                // wave-uniform fast path: no lane of the wave is within kmaxg tokens of a BREAK
                if (__all(run >= kmaxg)) sweep_token<KC, CANON, false>(win, run, kfirst, nk, p, s);
                else sweep_token<KC, CANON, true>(win, run, kfirst, nk, p, s);
            }
        });
    }
    if (s.dense) sweep_drain(s);
    __syncthreads();

    // merge the group's registers into the genome's slab (rows krow .. krow+nk-1 are contiguous)
    const uint4* l4 = reinterpret_cast<const uint4*>(g_lds);
    uint32_t* gw = reinterpret_cast<uint32_t*>(slab);
    const uint32_t n16 = (uint32_t)nk * (m >> 4);
    // Saturation: mx, the value that stands in the slab word when this thread leaves it, is compared with the universe word.
    // A slab word only ever grows and never passes the universe word, so a stale `old` cannot make a word look equal that
    // is not.  short_rows: bit j = this thread saw a word of row j below its universe word.
    const uint32_t nsat16 = (uint32_t)nsat * (m >> 4);
    const uint8_t* const urow = universe + ((size_t)(kfirst - kSatMinK) << p);
    uint32_t short_rows = 0;
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) {
        const uint4 lv = l4[i];
        const uint4 gv = load16_fresh(slab + (size_t)i * 16);
        const uint32_t l[4] = {lv.x, lv.y, lv.z, lv.w};
        const uint32_t o[4] = {gv.x, gv.y, gv.z, gv.w};
        uint32_t u[4] = {0u, 0u, 0u, 0u}, below = 0;
        if (KC == 0 && i < nsat16) {
            const uint4 uv = gload16(urow + (size_t)i * 16);
            u[0] = uv.x, u[1] = uv.y, u[2] = uv.z, u[3] = uv.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t old = o[q];
            uint32_t mx = bmax4(old, l[q]);
            while (mx != old) {
                uint32_t prev = gcas32(&gw[4 * i + q], old, mx);
                if (prev == old) break;
                old = prev;
                mx = bmax4(old, l[q]);
            }
            below |= mx ^ u[q];
        }
        if (KC == 0 && i < nsat16 && below) short_rows |= 1u << (i >> (p - 4));
    }
    if constexpr (KC == 0) {
        if (nsat) {
            // no word of a row below over the whole workgroup: the row is final.  (The OR goes through a word of g_lds, once
            // every thread has read its registers.  The flag is raised by an agent-scope atomic: a plain store would stay
            // in this XCD's L2, out of sight of the other seven's flag reads.)
            uint32_t* const word = reinterpret_cast<uint32_t*>(g_lds);
            __syncthreads();
            if (threadIdx.x == 0) *word = 0u;
            __syncthreads();
            if (short_rows) atomicOr(word, short_rows);
            __syncthreads();
            if (threadIdx.x < (uint32_t)nsat && !((*word >> threadIdx.x) & 1u)) gor32(g.sat + krow + threadIdx.x, 1u);
        }
    }
}

// ---- small-k class (k <= kBitmapMaxK): presence bitmaps instead of hashing every occurrence -----
// The sketch depends only on the SET of canonical k-mers, and for k <= 9 that set has at most
// 4^9 members, so per (token, k) this kernel only does: mask/shift, canonical min, one LDS word
// read and a bit test (an LDS atomic OR the first time a k-mer is seen).  bitmap_finish_kernel then
// hashes each recorded k-mer exactly once.  Registers are bit-identical to hashing every occurrence.
__constant__ int c_bitmap_off[kBitmapMaxK + 2] = {0, bitmap_offset(1), bitmap_offset(2), bitmap_offset(3),
                                                 bitmap_offset(4), bitmap_offset(5), bitmap_offset(6),
                                                 bitmap_offset(7), bitmap_offset(8), bitmap_offset(9),
                                                 kBitmapWords};
static_assert(kBitmapMaxK == 9 && bitmap_offset(9) + bitmap_words(9) == kBitmapWords &&
              kBitmapWords + kBitmapMaxK < kBitmapStride, "bitmap layout");

// amdgpu_num_sgpr: above 80 SGPRs only 7 waves per SIMD are admitted, i.e. ONE 1024-thread
// workgroup per CU instead of two (MI355X_MICROARCH.md, residency) -- measured 2x on this kernel.
template <bool CANON>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(72))) void bitmap_kernel(const SweepGenome* __restrict__ genomes,
                                                     const SweepJob* __restrict__ jobs) {
    const SweepJob job = jobs[blockIdx.x];
    const SweepGenome g = genomes[job.genome];
    const int kfirst = job.kfirst, klast = job.kfirst + job.nk - 1;
    const unsigned long long ntok = gload8u(g.ntok);
    const int w0 = c_bitmap_off[kfirst], w1 = c_bitmap_off[klast + 1];
    // the LDS image holds words w0..w1-1 of the genome's bitmap block, addressed by their global index
    uint32_t* const bits = reinterpret_cast<uint32_t*>(g_lds) - w0;
    uint32_t kmask = __builtin_amdgcn_readfirstlane(((2u << klast) - 1u) & ~((1u << kfirst) - 1u));  // bit k set: k in the job
    // A k whose set is COMPLETE -- every possible (canonical) k-mer already recorded, which small k
    // reach within the first few hundred thousand tokens of any genome -- can gain nothing from more
    // tokens.  The job that first sees a complete set (below, and again after its merge) raises a flag
    // behind the genome's bitmaps; a job that finds all its ks flagged returns before loading anything.
    uint32_t* const complete = g.bitmap + kBitmapWords;  // one word per k (the block's slack, zeroed per call)
    // warm start from what earlier jobs recorded (any snapshot is a subset of the final set), counting
    // the k-mers each k already has
    __shared__ uint32_t have[kBitmapMaxK + 2];
    __shared__ uint32_t flagged;
    // ONE thread reads the flags for the workgroup: another workgroup may set a flag at any moment, and waves
    // that read it at different times would disagree on kmask -- some would return while others go on to read
    // LDS words the returned waves were meant to load.  The reader is the first WAVE: lane k loads the flag of k, all of the
    // job's flags in one round trip (most workgroups of a big call do nothing but this), and the ballot is the one reading.
    if (threadIdx.x < 64) {
        const int k = (int)threadIdx.x;
        const uint32_t v = (k >= kfirst && k <= klast) ? load4_fresh(complete + k) : 0u;
        const unsigned long long f = __ballot(v != 0u);
        if (threadIdx.x == 0) flagged = (uint32_t)f;
    }
    if (threadIdx.x <= kBitmapMaxK) have[threadIdx.x] = 0;
    __syncthreads();
    kmask = __builtin_amdgcn_readfirstlane(kmask & ~flagged);
    if (kmask == 0u) return;
    for (int i = w0 + (int)threadIdx.x; i < w1; i += blockDim.x) {
        const uint32_t v = load4_fresh(&g.bitmap[i]);
        bits[i] = v;
        if (v) {
            int k = kfirst;
            for (int j = kfirst + 1; j <= klast; ++j) k = (i >= c_bitmap_off[j]) ? j : k;
            atomicAdd(&have[k], (uint32_t)__builtin_popcount(v));
        }
    }
    __syncthreads();
    auto all_of = [](int k) { return CANON ? (1u << (2 * k - 1)) + ((k & 1) ? 0u : (1u << (k - 1))) : (1u << (2 * k)); };
    for (int k = kfirst; k <= klast; ++k) {
        if (have[k] == all_of(k)) {
            kmask &= ~(1u << k);
            if (threadIdx.x == 0) gstore4(complete + k, 1u);
        }
    }
    kmask = __builtin_amdgcn_readfirstlane(kmask);
    if (kmask == 0u) return;

    const int prime = klast - 1;
    for (unsigned tile = job.tile_begin; tile < job.tile_end; ++tile) {
        const unsigned long long seg = (unsigned long long)tile * blockDim.x + threadIdx.x;
        if (seg * kSegTokens >= ntok) continue;
        SmallWindows<true> win{};
        const SmallIn in = fetch_small(g, seg, prime, win);
        const uint4 sc = in.sc;
        const uint2 sb = in.sb;
        int run = in.run;
        const uint32_t cws[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t bw = ((w & 2) ? sb.y : sb.x) >> ((w & 1) * 16);
#pragma unroll 1
            for (int i = 0; i < 16; ++i) {
                const uint32_t c = (cws[w] >> (2 * i)) & 3u;
                run = ((bw >> i) & 1u) ? 0 : run + 1;
                win.push(c);
                // fully unrolled over k so masks, shifts and bitmap offsets are immediates and the
                // LDS word reads of all ks are in flight together; `need` collects the (rare) lanes
                // that saw a new k-mer
                uint32_t xs[kBitmapMaxK + 1], seen[kBitmapMaxK + 1];
                uint32_t all_seen = 1u;  // bit 0 stays set while every k-mer of this token is known
#pragma unroll
                for (int k = 1; k <= kBitmapMaxK; ++k) {
                    if (!((kmask >> k) & 1u)) continue;  // wave-uniform (one scalar bit test, no live SGPR pair per k)
                    uint32_t x = win.fw & ((1u << (2 * k)) - 1u);
                    if (CANON) {
                        const uint32_t r = win.rc >> (32 - 2 * k);
                        x = x < r ? x : r;
                    }
                    xs[k] = x;
                    seen[k] = bits[bitmap_offset(k) + (x >> 5)];
                    all_seen &= seen[k] >> (x & 31u);
                }
                // Validity (run >= k) is only consulted on the rare path: an invalid window near a
                // BREAK can at worst send its lane there for nothing.
                if (!(all_seen & 1u)) {
#pragma unroll
                    for (int k = 1; k <= kBitmapMaxK; ++k) {
                        if (!((kmask >> k) & 1u) || run < k) continue;
                        if (!((seen[k] >> (xs[k] & 31u)) & 1u))
                            atomicOr(&bits[bitmap_offset(k) + (xs[k] >> 5)], 1u << (xs[k] & 31u));
                    }
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x <= kBitmapMaxK) have[threadIdx.x] = 0;
    __syncthreads();
    for (int i = w0 + (int)threadIdx.x; i < w1; i += blockDim.x) {
        const uint32_t mine = bits[i], theirs = load4_fresh(&g.bitmap[i]);
        if (mine & ~theirs) gor32(&g.bitmap[i], mine);
        int k = kfirst;
        for (int j = kfirst + 1; j <= klast; ++j) k = (i >= c_bitmap_off[j]) ? j : k;
        if (mine | theirs) atomicAdd(&have[k], (uint32_t)__builtin_popcount(mine | theirs));
    }
    __syncthreads();
    if (threadIdx.x >= (unsigned)kfirst && threadIdx.x <= (unsigned)klast && have[threadIdx.x] == all_of((int)threadIdx.x))
        gstore4(complete + threadIdx.x, 1u);
}

// grid = (ks, genomes, index tiles): a workgroup builds one 64 KiB tile of the row in LDS (the whole row when it is
// smaller) from ALL the k-mers of the set -- hashing a k-mer 16 times at log2m 20 costs nothing next to what one
// workgroup per row doing global compare-and-swaps cost there (2.3 ms for the k = 9 rows alone).
__global__ __launch_bounds__(1024) void bitmap_finish_kernel(const SweepGenome* __restrict__ genomes,
                                                            int kfirst, int kmin, int p, int tile_log2) {
    lds_starts_at_zero();
    const SweepGenome g = genomes[blockIdx.y];
    const int k = kfirst + (int)blockIdx.x;
    const uint32_t b = blockIdx.z;
    const uint32_t* bm = g.bitmap + c_bitmap_off[k];
    const uint32_t nw = (uint32_t)(c_bitmap_off[k + 1] - c_bitmap_off[k]);
    uint8_t* const row = g.regs + ((size_t)(k - kmin) << p);
    if (gridDim.z > 1 && nw <= 512) {
        // k <= 7 in a row of several tiles: at most 8256 k-mers for a row of 2^17 .. 2^20 registers that the call
        // zeroed when it started -- ONE workgroup raises the few registers in place instead of 16 writing tiles of
        // zeros (64 genomes at log2m 20: 4096 of the launch's 6144 workgroups)
        if (b != 0) return;
        for_each_set_bit(bm, nw, [&](uint32_t x) { hll_update(RegsGlobal{row}, wang64_fast<true>(x), p); });
        return;
    }
    // (the set's bit index is the k-mer)
    finish_tile(row + ((size_t)b << tile_log2), tile_log2, b, p, [&](const auto& emit) { for_each_set_bit(bm, nw, emit); });
}


// ---- big-bitmap class (dd_kernels.h): k = 10 (, 11) at log2m >= 19 ---------------------------------------
// index of the k-mer whose forward / reverse-complement values are fw / rc (both 2k bits)
template <bool CANON>
DD_D uint32_t bigmap_index(uint32_t fw, uint32_t rc, int k) {
    if (!CANON) return fw;
    if (k & 1) {
        const uint32_t y = ((fw >> k) & 1u) ? rc : fw;  // the strand whose middle base is A or C
        return ((y >> (k + 1)) << k) | (y & ((1u << k) - 1u));
    }
    return fw < rc ? fw : rc;
}
// ... and back: the value that is hashed
template <bool CANON>
DD_D uint32_t bigmap_kmer(uint32_t idx, int k) {
    if (!CANON || !(k & 1)) return idx;
    const uint32_t y = ((idx >> k) << (k + 1)) | (idx & ((1u << k) - 1u));
    uint32_t r = __brev(y);                                        // bases reversed, the two bits of each swapped
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    r = (~r) >> (32 - 2 * k);
    return y < r ? y : r;
}

// One workgroup per CU (128 KiB of LDS): the slice as earlier jobs left it, this job's tiles, merge.
template <bool CANON>
__global__ __launch_bounds__(1024) void bigmap_kernel(const SweepGenome* __restrict__ genomes, const SweepJob* __restrict__ jobs) {
    const SweepJob job = jobs[blockIdx.x];
    const SweepGenome g = genomes[job.genome];
    const int k = job.kfirst;
    const uint32_t slice = (uint32_t)job.slice;
    const unsigned long long ntok = gload8u(g.ntok);
    uint32_t* const home = g.bigmap + bigmap_offset_words(k, CANON) + (size_t)slice * kBigmapSliceWords;
    uint32_t* const bits = reinterpret_cast<uint32_t*>(g_lds);
    for (int i = threadIdx.x; i < kBigmapSliceWords; i += blockDim.x) bits[i] = load4_fresh(home + i);
    __syncthreads();
    const uint32_t mask = (1u << (2 * k)) - 1u;
    const int top = 2 * k - 2, prime = k - 1;
    for (unsigned tile = job.tile_begin; tile < job.tile_end; ++tile) {
        const unsigned long long seg = (unsigned long long)tile * blockDim.x + threadIdx.x;
        if (seg * kSegTokens >= ntok) continue;
        SmallWindows<false> win{mask, top};
        const SmallIn in = fetch_small(g, seg, prime, win);
        const uint4 sc = in.sc;
        const uint2 sb = in.sb;
        int run = in.run;
        const uint32_t cws[4] = {sc.x, sc.y, sc.z, sc.w};
        auto record = [&](uint32_t idx, bool ok) {
            if ((idx >> 20) == slice && ok) {
                const uint32_t at = (idx & 0xFFFFFu) >> 5, bit = 1u << (idx & 31u);
                if (!(bits[at] & bit)) atomicOr(&bits[at], bit);
            }
        };
        if (__all((sb.x | sb.y) == 0u && run >= prime)) {
            // the usual case: no BREAK anywhere in the wave's 64 x 64 tokens, every window valid
#pragma unroll
            for (int w = 0; w < 4; ++w) {
#pragma unroll 4
                for (int i = 0; i < 16; ++i) {
                    const uint32_t c = (cws[w] >> (2 * i)) & 3u;
                    win.push(c);
                    record(bigmap_index<CANON>(win.fw, win.rc, k), true);
                }
            }
            continue;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t bw = ((w & 2) ? sb.y : sb.x) >> ((w & 1) * 16);
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const uint32_t c = (cws[w] >> (2 * i)) & 3u;
                run = ((bw >> i) & 1u) ? 0 : run + 1;
                win.push(c);
                record(bigmap_index<CANON>(win.fw, win.rc, k), run >= k);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBigmapSliceWords; i += blockDim.x) {
        const uint32_t mine = bits[i];
        if (mine && (mine & ~load4_fresh(home + i))) gor32(home + i, mine);
    }
}

// grid = (ks, genomes, index tiles), as bitmap_finish_kernel
template <bool CANON>
__global__ __launch_bounds__(1024) void bigmap_finish_kernel(const SweepGenome* __restrict__ genomes,
                                                            int kfirst, int kmin, int p, int tile_log2) {
    lds_starts_at_zero();
    const SweepGenome g = genomes[blockIdx.y];
    const int k = kfirst + (int)blockIdx.x;
    const uint32_t b = blockIdx.z;
    const uint32_t* bm = g.bigmap + bigmap_offset_words(k, CANON);
    const uint32_t nw = (uint32_t)bigmap_slices(k, CANON) * kBigmapSliceWords;
    finish_tile(g.regs + ((size_t)(k - kmin) << p) + ((size_t)b << tile_log2), tile_log2, b, p, [&](const auto& emit) {
        for_each_set_bit(bm, nw, [&](uint32_t idx) { emit(bigmap_kmer<CANON>(idx, k)); });
    });
}

// ---- saturation: sketch(U_k), the row every (canonical) k-mer hashed once gives (dd_kernels.h) ------------------------------
// Each workgroup hashes its share of x in [0, 4^k) -- in canonical mode only the x that are the smaller of (x, reverse
// complement), which is what sweep_kernel hashes -- into a row in LDS and byte-max-merges it into the row in HBM (zeroed by the
// launcher), as sweep_kernel merges its groups.
template <bool CANON>
__global__ __launch_bounds__(1024) void universe_kernel(uint8_t* __restrict__ row, int k, int p) {
    lds_starts_at_zero();
    const uint32_t m = 1u << p;
    uint4* z = reinterpret_cast<uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < (m >> 4); i += blockDim.x) z[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t n = 1u << (2 * k);  // k <= kSatMaxK = 14
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        if (CANON) {
            uint32_t r = __brev(x);  // bases reversed, the two bits of each swapped
            r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
            r = (~r) >> (32 - 2 * k);
            if (r < x) continue;
        }
        const Probe q = probe(wang64_fast<true>(x), p);
        lds_raise(q.hi >> (32 - p), rho_of(q, p));
    }
    __syncthreads();
    const uint4* l4 = reinterpret_cast<const uint4*>(g_lds);
    uint32_t* gw = reinterpret_cast<uint32_t*>(row);
    for (uint32_t i = threadIdx.x; i < (m >> 4); i += blockDim.x) {
        const uint4 lv = l4[i];
        const uint4 gv = load16_fresh(row + (size_t)i * 16);
        const uint32_t l[4] = {lv.x, lv.y, lv.z, lv.w};
        const uint32_t o[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t old = o[q];
            uint32_t mx = bmax4(old, l[q]);
            while (mx != old) {
                uint32_t prev = gcas32(&gw[4 * i + q], old, mx);
                if (prev == old) break;
                old = prev;
                mx = bmax4(old, l[q]);
            }
        }
    }
}

}  // namespace

void launch_universe(uint8_t* row_dev, int k, int log2m, int canonical, hipStream_t st) {
    if (k < kSatMinK || k > kSatMaxK || log2m < 4 || log2m > 16) return;
    (void)hipMemsetAsync(row_dev, 0, (size_t)1 << log2m, st);
    // 2^16 k-mers per workgroup, 1024 workgroups at the most (k = 14: 2^18 each)
    const unsigned grid = std::min(1024u, 1u << (2 * k - 16));
    dispatch_bool(canonical != 0, [&](auto cn) {
        hipLaunchKernelGGL(universe_kernel<decltype(cn)::value>, dim3(grid), dim3(1024), (size_t)1 << log2m, st, row_dev, k, log2m);
    });
}

int sweep_max_lds_bytes() { return 160 * 1024; }

void launch_bitmap(const SweepGenome* genomes, const SweepJob* jobs, int njobs, int kfirst, int klast,
                   int canonical, hipStream_t st) {
    if (njobs <= 0 || kfirst < 1 || klast > kBitmapMaxK || klast < kfirst) return;
    const size_t lds = (size_t)(bitmap_offset(klast) + bitmap_words(klast) - bitmap_offset(kfirst)) * 4;
    dispatch_bool(canonical != 0, [&](auto cn) {
        launch_full_lds<bitmap_kernel<decltype(cn)::value>, 256>(dim3((unsigned)njobs), dim3(1024), lds, st, genomes, jobs);
    });
}

void launch_bitmap_finish(const SweepGenome* genomes, int ngenomes, int kfirst, int klast, int kmin, int log2m,
                          hipStream_t st) {
    if (ngenomes <= 0 || klast < kfirst) return;
    const int tile_log2 = std::min(log2m, 16);
    hipLaunchKernelGGL(bitmap_finish_kernel, dim3((unsigned)(klast - kfirst + 1), (unsigned)ngenomes, 1u << (log2m - tile_log2)), dim3(1024),
                       (size_t)1 << tile_log2, st, genomes, kfirst, kmin, log2m, tile_log2);
}

void launch_bigmap(const SweepGenome* genomes, const SweepJob* jobs, int njobs, int canonical, hipStream_t st) {
    if (njobs <= 0) return;
    dispatch_bool(canonical != 0, [&](auto cn) {
        launch_full_lds<bigmap_kernel<decltype(cn)::value>>(dim3((unsigned)njobs), dim3(1024), (size_t)kBigmapSliceWords * 4, st, genomes, jobs);
    });
}

void launch_bigmap_finish(const SweepGenome* genomes, int ngenomes, int kfirst, int klast, int kmin, int log2m,
                          int canonical, hipStream_t st) {
    if (ngenomes <= 0 || klast < kfirst) return;
    // 128 KiB tiles, one workgroup per CU: every workgroup hashes the row's whole set (up to 2 M k-mers), so fewer,
    // larger tiles are less work
    const int tile_log2 = std::min(log2m, 17);
    const dim3 grid((unsigned)(klast - kfirst + 1), (unsigned)ngenomes, 1u << (log2m - tile_log2));
    dispatch_bool(canonical != 0, [&](auto cn) {
        launch_full_lds<bigmap_finish_kernel<decltype(cn)::value>>(grid, dim3(1024), (size_t)1 << tile_log2, st, genomes, kfirst, kmin, log2m, tile_log2);
    });
}

void launch_sweep(const SweepGenome* genomes, const SweepJob* jobs, int njobs, int kclass,
                  const SweepPlan& plan, const uint8_t* universe, int universe_last_k, hipStream_t st) {
    if (njobs <= 0) return;
    if (!universe || kclass != 0) universe_last_k = 0;
    dispatch_kc_canon(kclass, plan.canonical, [&](auto kc, auto cn) {
        launch_full_lds<sweep_kernel<decltype(kc)::value, decltype(cn)::value>>(dim3((unsigned)njobs), dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, st,
                                                                                genomes, jobs, plan.log2m, (uint32_t)plan.queue_off, universe, universe_last_k);
    });
}

}  // namespace dd
