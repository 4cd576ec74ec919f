// dd_exact_walk.h -- what more than one kernel of the exact device path does, once: the key masks of a k, the query test
// on a membership mask, the token walk of a 64-token segment (kmer_extract_kernel, locate_kernel, screen_kernel, paint_kernel,
// reads_kernel, depth_kernel, cover_index_kernel), the lookup of a key in the ordered records (locate_kernel, screen_kernel,
// paint_kernel, reads_kernel, depth_kernel, cover_index_kernel), the
// bit-sliced per-genome counter and its two flushes (paint_kernel, reads_kernel), the window a wave's counts go to
// (paint_kernel, cover_kernel), the wave-aggregated append (kmer_extract_kernel, sched_kernel, emit_kernel) and, on the host,
// the launch of a segment walk.  Everything here is inlined into its caller: no kernel calls across files.
#pragma once
#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {

// the masks of a k's key words: the low 2k bits of lo, the low 2k - 64 of hi
struct KeyMasks {
    uint64_t lo, hi;
};
DD_HD KeyMasks key_masks(int k) {
    return KeyMasks{(k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull), (k <= 32) ? 0ull : ((k == 64) ? ~0ull : ((1ull << (2 * k - 64)) - 1ull))};
}

// a query (all, none) on a membership mask: holds every genome of `all` and none of `none`
DD_HD bool mask_matches(uint64_t m, uint64_t all, uint64_t none) { return (m & all) == all && (m & none) == 0; }

// The token walk of one thread: segment `seg` (64 tokens) of a token stream of `ntok` tokens.  128-bit forward and
// reverse-complement windows serve every k <= 64; the segment in front warms them up (its k-mers belong to the thread in
// front), and a window is a k-mer once `run`, the tokens since the last BREAK, has reached k.  f(sidx, t, ah, al, have) is
// called for token t of segment sidx = seg with the k-mer that ends there under the key masks, (ah, al): the smaller of the
// two strands if CANON, the forward one if not.
//   EVERY = false: called at the tokens that end a k-mer only (have = true); a thread behind the stream returns at once.
//   EVERY = true:  called at every token of the segment, `have` saying whether a k-mer ends there, by every lane of a wave
//                  that has a live lane at all -- for a caller whose f is a wave-level operation.  The lanes behind the
//                  stream load nothing and walk BREAKs.
template <bool CANON, bool EVERY, class F>
DD_D void walk_segment(const uint32_t* codes, const uint32_t* bad, unsigned long long ntok, unsigned long long seg, int k, F&& f) {
    const bool live = seg * kSegTokens < ntok;
    if (EVERY ? !__any(live) : !live) return;
    const uint4* codes4 = reinterpret_cast<const uint4*>(codes);
    const uint2* bad2 = reinterpret_cast<const uint2*>(bad);
    uint64_t fh = 0, fl = 0, rh = 0, rl = 0;
    int run = 0;
    const KeyMasks km = key_masks(k);
    const int s = 128 - 2 * k;  // right shift that aligns the reverse-complement window
    for (int part = (seg > 0 ? 0 : 1); part < 2; ++part) {
        const unsigned long long sidx = seg - 1 + part;
        const uint4 c4 = (!EVERY || live) ? codes4[sidx] : make_uint4(0, 0, 0, 0);
        const uint2 b2 = (!EVERY || live) ? bad2[sidx] : make_uint2(~0u, ~0u);
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
            if (part == 0) continue;
            const bool have = run >= k;
            if (!EVERY && !have) continue;
            uint64_t ah = fh & km.hi, al = fl & km.lo;
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
            f(sidx, t, ah, al, have);
        }
    }
}

// Is (ah, al) one of the ordered records?  A lower_bound on (hi, lo): ceil(log2 found) dependent 8- or 16-byte reads, the
// first levels of which every thread shares (L2), then the exact-hit test.  `at`: the record on a hit.
template <bool WIDE>
DD_D bool find_record(const LocateSet& set, uint64_t ah, uint64_t al, unsigned long long& at) {
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
    at = first;
    if (first >= set.found || set.lo[first] != al) return false;
    return !WIDE || set.hi[first] == ah;
}

// the sum over the wave of a per-lane count below 2^kPaintPlanes, from one ballot per bit; the same in every lane
DD_D uint32_t wave_sum(uint32_t v) {
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kPaintPlanes; ++j) sum += (uint32_t)__builtin_popcountll(__ballot((v >> j) & 1u)) << j;
    return sum;
}

// The per-genome counter of a thread of paint_kernel and reads_kernel between two flushes: of the k-mers that are records,
// those whose mask has genome i's bit -- a bit-sliced VERTICAL counter, kPaintPlanes 64-bit planes, bit i of plane j = bit j
// of genome i's count.  A run of at most 64 k-mers: seven planes hold it.  A row is n + 2 columns: the k-mers that end
// (valid), those that are records (inpan), the genomes.  The two plain counts stay the kernel's own variables and come to the
// flushes as arguments: as members they cost reads_kernel 3 to 5 VGPRs (profiles/sample_entries_refactor.txt).
struct PlaneCounter {
    uint64_t p[kPaintPlanes];
    DD_D void clear() {
#pragma unroll
        for (int j = 0; j < kPaintPlanes; ++j) p[j] = 0;
    }
    // a k-mer that is a record with this mask: a ripple carry over the planes, no loop over genomes
    DD_D void add(uint64_t mask) {
        uint64_t carry = mask;
#pragma unroll
        for (int j = 0; j < kPaintPlanes; ++j) {
            const uint64_t both = p[j] & carry;
            p[j] ^= carry;
            carry = both;
        }
    }
    // genome i's count
    DD_D uint32_t count(int i) const {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < kPaintPlanes; ++j) c |= (uint32_t)((p[j] >> i) & 1ull) << j;
        return c;
    }
    // the thread's non-zero counts added to a row others add to
    DD_D void flush(uint32_t* row, int n, uint32_t valid, uint32_t inpan) const {
        if (valid) atomicAdd(row, valid);
        if (!inpan) return;
        atomicAdd(row + 1, inpan);
        for (int i = 0; i < n; ++i) {
            const uint32_t c = count(i);
            if (c) atomicAdd(row + 2 + i, c);
        }
    }
    // the whole wave's counts added to ONE row, by every lane of the wave (the lanes behind the stream hold zeros): column
    // i of plane j over the wave is one __ballot, lane i adds its popcount shifted by the plane's weight, and the wave
    // issues one no-return atomicAdd per non-zero column.  A plane that is zero in every lane costs one ballot.
    DD_D void flush_wave(uint32_t* row, int n, int lane, uint32_t valid, uint32_t inpan) const {
        const uint32_t v = wave_sum(valid), h = wave_sum(inpan);
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < kPaintPlanes; ++j) {
            const uint64_t pj = p[j];
            if (!__ballot(pj != 0)) continue;
            for (int i = 0; i < n; ++i) {
                const unsigned long long col = __ballot((pj >> i) & 1ull);
                if (lane == i) mine += (uint32_t)__builtin_popcountll(col) << j;
            }
        }
        if (lane < n && mine) atomicAdd(row + 2 + lane, mine);
        if (lane == 0 && v) atomicAdd(row, v);
        if (lane == 1 && h) atomicAdd(row + 1, h);
    }
};

// Do the live segments of a wave, 64 consecutive ones from `first` on, lie in ONE window of wsegs segments of a stream of
// ntok tokens (always so when the window is a multiple of 4096 tokens)?  The same in every lane.  w: that window.
// (paint_kernel, cover_kernel: where it is so the wave adds its counts to the window's row once, for all its lanes)
DD_D bool wave_in_one_window(unsigned long long first, unsigned long long ntok, unsigned long long wsegs, unsigned long long& w) {
    const unsigned long long end = (ntok - 1) / kSegTokens, last = first + 63 < end ? first + 63 : end;
    w = first / wsegs;
    return w == last / wsegs;
}

// Dense append by the lanes of a wave that `take`: one atomicAdd on the counter (uint32_t in LDS, unsigned long long in
// HBM) per wave, by the first taking lane, for all of them.  Returns the slot of a taking lane; the others get no slot.
// Called by every lane of the wave that is still running.
template <class T>
DD_D T wave_append(bool take, T* counter) {
    const unsigned long long mask = __ballot(take);
    if (!mask) return 0;
    const int leader = __builtin_ctzll(mask);
    const uint32_t lane = threadIdx.x & 63u;
    T base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (T)__builtin_popcountll(mask));
    base = __shfl(base, leader);
    return base + (T)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
}

// host: the launch of a kernel that walks segments -- one thread per 64-token segment of the longest stream, 256 to a
// workgroup, one launch unit (gridDim.y) per stream.  f(grid, block, canon, wide) launches the caller's kernel, the two
// std::bool_constants its template arguments.
template <class F>
void launch_segment_walk(size_t units, size_t max_segments, int canonical, int k, const F& f) {
    const dim3 grid((unsigned)((max_segments + 255) / 256), (unsigned)units), block(256);
    dispatch_bool(canonical != 0, [&](auto cn) { dispatch_bool(k > 32, [&](auto wd) { f(grid, block, cn, wd); }); });
}

}  // namespace dd
