// dd_k1.h -- what the sketching (K1) kernels of dd_sweep.hip and dd_scatter.hip share: the gfx950 forms of the hash, the
// register stores and the update, the rolling windows of every k class, a tile's input (one copy of the halo and segment
// loads), the walk over a segment's 64 tokens, the small-k classes' segment, the finish kernels' tile, and the host helpers
// that pick a <KC, CANON> instantiation and launch it.  Device code is DD_D or constexpr: no kernel calls across files.
#pragma once
#include "dd_common.h"
#include "dd_kernels.h"

#include <algorithm>
#include <type_traits>

namespace dd {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// The arithmetic of hash and probe is host-visible: the instruction forms are the device's, plain C the host's, so that
// tests/native/k1_hash.hip can run it against dd::wang64 and the definitions without a GPU.
DD_HD uint32_t ffbh(uint32_t x) {  // leading zeros; 0xFFFFFFFF for x == 0
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x ? (uint32_t)__builtin_clz(x) : ~0u;
#endif
}
DD_HD uint32_t mul_lo(uint32_t a, uint32_t c) {  // opaque to the optimiser: stays one v_mul_lo_u32
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_mul_lo_u32 %0, %1, %2" : "=v"(r) : "v"(a), "s"(c));
    return r;
#else
    return a * c;
#endif
}
// bits [s, s + 32) of hi:lo.  The count is taken modulo 32, as v_alignbit_b32 takes it: 32 gives lo, not hi.
DD_HD uint32_t funnel32(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31));
#endif
}
template <int SH>
DD_HD uint64_t lshl_add64(uint64_t a, uint64_t b) {  // (a << SH) + b, SH in 0..4, one instruction
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r;
    asm("v_lshl_add_u64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(SH), "v"(b));
    return r;
#else
    return (a << SH) + b;
#endif
}
// x * C + addend (mod 2^64), C a 32-bit constant: v_mad_u64_u32 + v_mul_lo_u32 + v_add_u32 (HI_ZERO, x < 2^32: the mad alone)
template <bool HI_ZERO>
DD_HD uint64_t mul64_c32(uint64_t x, uint32_t C, uint64_t addend) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint64_t pr = (uint64_t)lo * C + addend;
    if (HI_ZERO) return pr;
    const uint32_t ph = (uint32_t)(pr >> 32) + mul_lo(hi, C);
    return ((uint64_t)ph << 32) | (uint32_t)pr;
}
// x * C (mod 2^64) with nothing to add: the high product goes in as the mad's addend, lo * C + (mul_lo(hi, C) << 32) --
// v_mul_lo_u32 writes the odd half of a register pair whose even half stays zero, v_mad_u64_u32 takes the pair as src2, and
// the v_add_u32 of mul64_c32 is gone.  (Not for x * (2^21 - 1) - 1: the high word of that addend would be hi * C - 1, and
// every way to it -- (hi << 21) + ~hi, the modular inverse, a 64-bit -1 behind -- costs the instruction back.)
DD_HD uint64_t mul64_c32_fold(uint64_t x, uint32_t C) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    return (uint64_t)lo * C + ((uint64_t)mul_lo(hi, C) << 32);
}

// Thomas Wang 64-bit mix, identical to dd::wang64 (tests/native/k1_hash.hip on the host; asserted on every lane by the
// GPU parity tests), arranged for the gfx950 issue costs (dd_sweep.hip, head): 18 instructions, 16 for HI_ZERO.
template <bool HI_ZERO>
DD_HD uint64_t wang64_fast(uint64_t x) {
    x = mul64_c32<HI_ZERO>(x, 0x1FFFFFu, ~0ull);  // ~x + (x << 21) = x * (2^21 - 1) - 1
    x ^= x >> 24;
    x = mul64_c32_fold(x, 265u);                  // x + (x << 3) + (x << 8)
    x ^= x >> 14;
    x = lshl_add64<2>(lshl_add64<2>(x, x), x);    // x + (x << 2) + (x << 4) = ((5x) << 2) + x
    x ^= x >> 28;
    return lshl_add64<0>(x << 31, x);             // x + (x << 31)
}

// ---- register stores -------------------------------------------------------------------------
// kernels that address LDS absolutely (RegsLds, scatter_update's filter read) call this first
DD_D void lds_starts_at_zero() {
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)g_lds != 0u) __builtin_trap();
}

// LDS: byte registers, 32-bit compare-and-swap on the containing word when a register must rise.
struct RegsLds {
    uint32_t slot;  // the slot's registers start at byte slot << p of g_lds
    using Addr = uint32_t;
    // address of register  hi >> (32-p)  (the top p bits of the hash): one v_alignbit of slot:hi
    DD_HD Addr at(uint32_t hi, int p) const { return funnel32(slot, hi, 32u - (uint32_t)p); }
    DD_D static uint32_t shift(Addr a) { return (a & 3u) * 8u; }
    // Registers are read at their ABSOLUTE LDS address: every kernel that uses this struct has no static LDS, so the
    // dynamic array g_lds starts at 0 (lds_starts_at_zero() at the top of each checks it), and indexing through the
    // g_lds symbol would cost a `v_add_u32 v, 0, v` of its link-time address on every read -- 1.5 of the 31.5 VALU
    // instructions of a k 17..32 update at log2m <= 16.
    DD_D uint32_t bound(Addr a) const { return *(const __attribute__((address_space(3))) uint8_t*)(uintptr_t)a; }  // the register itself
    DD_D static uint32_t load32(Addr a) { return *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)(a & ~3u); }
    DD_D static uint32_t cas32(Addr a, uint32_t expect, uint32_t desired) {
        return atomicCAS(reinterpret_cast<uint32_t*>(g_lds + (a & ~3u)), expect, desired);
    }
};
// HBM/L2: same protocol on the genome's slab (p >= 18: one array no longer fits LDS).
struct RegsGlobal {
    uint8_t* base;  // 16-byte aligned
    using Addr = uint8_t*;
    DD_D Addr at(uint32_t hi, int p) const { return base + (hi >> (32 - p)); }
    DD_D static uint32_t shift(Addr a) { return ((uint32_t)(uintptr_t)a & 3u) * 8u; }
    DD_D static uint8_t* word(Addr a) {
        return static_cast<uint8_t*>(__builtin_assume_aligned(a - ((uintptr_t)a & 3u), 4));
    }
    DD_D uint32_t bound(Addr a) const { return gload1_fresh(a); }
    DD_D static uint32_t load32(Addr a) { return gload4_fresh(word(a)); }
    DD_D static uint32_t cas32(Addr a, uint32_t expect, uint32_t desired) { return gcas32(word(a), expect, desired); }
};

// 16 bytes of global memory as other agents' atomics left them (two relaxed agent-scope 8-byte
// loads: they bypass this XCD's non-coherent L2).
DD_D uint4 load16_fresh(const uint8_t* p) {
    const uint8_t* q = static_cast<const uint8_t*>(__builtin_assume_aligned(p, 16));
    const unsigned long long a = gload8_fresh(q), b = gload8_fresh(q + 8);
    return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}
DD_D uint32_t load4_fresh(const uint32_t* p) { return gload4_fresh(p); }

// hi = top word of h (its top p bits index the register) and lz = rho(h) - 1 (0xFFFFFFFF when the
// top 32 bits of h << p are all zero)
struct Probe {
    uint32_t hi, lz, hiw, lo;
};
DD_HD Probe probe(uint64_t h, int p) {
    const uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
    Probe r;
    r.hi = hi;
    r.hiw = funnel32(hi, lo, 32u - (uint32_t)p);  // bits 63..32 of (h << p)
    r.lz = ffbh(r.hiw);
    r.lo = lo;
    return r;
}
// rho(h) from a probe: lz + 1, in its long form only when the 32 bits after the index are all zero
// (p = 2^-32: behind a wave-level branch)
DD_D uint32_t rho_of(const Probe& q, int p) {
    uint32_t rho = q.lz + 1;  // 0 where hiw == 0
    if (__builtin_expect(__any(q.hiw == 0), 0)) {
        if (q.hiw == 0) rho = 33u + (uint32_t)__builtin_clz((q.lo << p) | (1u << (p - 1)));
    }
    return rho;
}
// Exact byte-max of rho into the register at `a` through a 32-bit CAS on the containing word,
// starting from the word value `old`; returns the register's value afterwards.  The byte is raised by
// ADDING (rho - cur) << shift: no carry can leave the byte.
template <typename R>
DD_D uint32_t cas_raise(typename R::Addr a, uint32_t old, uint32_t rho) {
    const uint32_t sh = R::shift(a);
    while (true) {
        const uint32_t cur = (old >> sh) & 0xFFu;
        if (rho <= cur) return cur;
        const uint32_t prev = R::cas32(a, old, old + ((rho - cur) << sh));
        if (prev == old) return rho;
        old = prev;
    }
}
// The rare path: the register at `a` was seen below rho.  Every instruction here is paid by the
// whole wave for (typically) one lane, so it is kept short.
template <typename R>
DD_D void raise(const R&, typename R::Addr a, const Probe& q, int p) {
    (void)cas_raise<R>(a, R::load32(a), rho_of(q, p));
}

DD_D uint32_t min4(uint32_t w) {  // smallest byte
    const uint32_t a = w & 0xFFu, b = (w >> 8) & 0xFFu, c = (w >> 16) & 0xFFu, d = w >> 24;
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}
// reg[h >> (64-p)] = max(., rho(h)); the common case (no change) is one byte read + compare.
template <typename R>
DD_D void hll_update(const R& regs, uint64_t h, int p) {
    const Probe q = probe(h, p);
    const typename R::Addr a = regs.at(q.hi, p);
    if (q.lz >= regs.bound(a)) raise(regs, a, q, p);  // rho > bound, or hiw == 0 (resolved there)
}
// two independent updates interleaved: both hash chains and both LDS reads are in flight
// together, one wave-level branch covers the common no-change case of both
template <typename R>
DD_D void hll_update2(const R& r0, uint64_t h0, const R& r1, uint64_t h1, int p) {
    const Probe qa = probe(h0, p), qb = probe(h1, p);
    const typename R::Addr a = r0.at(qa.hi, p), b = r1.at(qb.hi, p);
    const uint32_t c0 = r0.bound(a), c1 = r1.bound(b);
    if ((qa.lz >= c0) | (qb.lz >= c1)) {
        if (qa.lz >= c0) raise(r0, a, qa, p);
        if (qb.lz >= c1) raise(r1, b, qb, p);
    }
}

// ---- sweep_kernel's raises: queued per wave, applied 64 at a time ------------------------------------------------------
// A candidate (lz >= the register's byte) does not run raise()'s load / compare-and-swap sequence -- some twenty wave
// instructions and two LDS round trips for, typically, one lane: the lane appends a record
// (LDS byte address | (rho - 1) << 24) to its WAVE's queue behind the group's registers (dd_plan.hip makes the room), and once
// 64 wait they are applied one per lane.  Exact: cas_raise is a byte-max, so a record that names a register raised since,
// or one named twice, changes nothing; probes in between see a stale (lower) byte, which only makes more candidates.
// Capacity: a wave applies 64 records as soon as 64 wait, so an append finds at most 63, and one step (a k pair) adds at
// most 31 -- kRaiseDense or more candidate lanes, as in every step of a cold job, are applied at once, not queued: never
// more than 94 of the kRaiseQueueRecords (dd_kernels.h).  Every function here is reached by whole waves.
constexpr uint32_t kRaiseDense = 32;
static_assert(63 + (kRaiseDense - 1) <= kRaiseQueueRecords, "raise queue capacity");

struct RaiseQueue {
    uint32_t base;     // LDS byte address of this wave's records
    uint32_t dense;    // kRaiseDense, or 0: no queue (the 32-bit class; a group that left no room), every raise is applied at once
    uint32_t waiting;  // records in the queue (wave-uniform)
};
DD_D uint32_t lds_load32(uint32_t a) { return *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)a; }  // (absolute, as RegsLds)
DD_D void lds_store32(uint32_t a, uint32_t v) { *(__attribute__((address_space(3))) uint32_t*)(uintptr_t)a = v; }
DD_D void raise_record(uint32_t rec) {
    const uint32_t a = rec & 0xFFFFFFu;
    (void)cas_raise<RegsLds>(a, RegsLds::load32(a), (rec >> 24) + 1u);
}
// rho - 1 from a probe, in its long form where the 32 bits after the index are all zero (rho_of)
DD_D uint32_t rho_minus_1(const Probe& q, int p) {
    return q.lz != ~0u ? q.lz : 32u + (uint32_t)__builtin_clz((q.lo << p) | (1u << (p - 1)));
}
// Behind the wave-level "any candidate" branch of one or two updates: the lanes of m0 (c0: this lane is one) must raise
// their register at a to rho(qa), those of m1 theirs at b to rho(qb).
template <bool QUEUE>
DD_D void sweep_raise(RaiseQueue& s, int p, unsigned long long m0, bool c0, uint32_t a, const Probe& qa,
                      unsigned long long m1, bool c1, uint32_t b, const Probe& qb) {
    uint32_t z0 = qa.lz, z1 = qb.lz;
    if (__builtin_expect(__any((int32_t)(z0 | z1) < 0), 0)) {  // (lz is <= 31 or 0xFFFFFFFF)
        z0 = rho_minus_1(qa, p);
        z1 = rho_minus_1(qb, p);
    }
    const uint32_t n0 = (uint32_t)__builtin_popcountll(m0), n = n0 + (uint32_t)__builtin_popcountll(m1);
    if (QUEUE && n < s.dense) {
        // (one scalar, so that a lane's slot is one v_lshl_add of its rank)
        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane(s.base + 4u * s.waiting);
        if (c0) lds_store32(at + 4u * lanes_below(m0), a | (z0 << 24));
        if (c1) lds_store32((uint32_t)__builtin_amdgcn_readfirstlane(at + 4u * n0) + 4u * lanes_below(m1), b | (z1 << 24));
        s.waiting += n;
        if (s.waiting >= 64u) {
            s.waiting -= 64u;
            raise_record(lds_load32(s.base + 4u * (s.waiting + lanes_below(~0ull))));
        }
        return;
    }
    if (c0) (void)cas_raise<RegsLds>(a, RegsLds::load32(a), z0 + 1u);
    if (c1) (void)cas_raise<RegsLds>(b, RegsLds::load32(b), z1 + 1u);
}
// what still waits when the job's tiles are done
DD_D void sweep_drain(RaiseQueue& s) {
    const uint32_t lane = lanes_below(~0ull);
    if (lane < s.waiting) raise_record(lds_load32(s.base + 4u * lane));
    s.waiting = 0;
}
// hll_update / hll_update2 on the group's LDS registers.  MASKED (the walk's CHECK variant): only for the lanes with ok
// (okm: its ballot, taken by the caller beside the compare).
// The candidate masks are the ballots of the plain compares, combined as scalars: the ballot of a combined condition
// costs a v_cndmask + v_cmp pair per update, in the loop every update runs.
template <bool QUEUE, bool MASKED>
DD_D void sweep_update(RaiseQueue& s, uint32_t slot, uint64_t h, unsigned long long okm, bool ok, int p) {
    const RegsLds regs{slot};
    const Probe q = probe(h, p);
    const uint32_t a = regs.at(q.hi, p);
    const bool r = q.lz >= regs.bound(a);
    unsigned long long mask = __builtin_amdgcn_ballot_w64(r);
    if (MASKED) mask &= okm;
    if (mask) sweep_raise<QUEUE>(s, p, mask, MASKED ? (ok & r) : r, a, q, 0ull, false, 0u, Probe{0u, 0u, 0u, 0u});
}
template <bool QUEUE, bool MASKED>
DD_D void sweep_update2(RaiseQueue& s, uint32_t slot0, uint64_t h0, unsigned long long okm0, bool ok0,
                        uint32_t slot1, uint64_t h1, unsigned long long okm1, bool ok1, int p) {
    const RegsLds r0{slot0}, r1{slot1};
    const Probe qa = probe(h0, p), qb = probe(h1, p);
    const uint32_t a = r0.at(qa.hi, p), b = r1.at(qb.hi, p);
    const uint32_t v0 = r0.bound(a), v1 = r1.bound(b);
    const bool c0 = qa.lz >= v0, c1 = qb.lz >= v1;
    unsigned long long m0 = __builtin_amdgcn_ballot_w64(c0), m1 = __builtin_amdgcn_ballot_w64(c1);
    if (MASKED) m0 &= okm0, m1 &= okm1;
    if (m0 | m1) sweep_raise<QUEUE>(s, p, m0, MASKED ? (ok0 & c0) : c0, a, qa, m1, MASKED ? (ok1 & c1) : c1, b, qb);
}

// Reverse the order of the 16 2-bit fields of a code word: the token stream stores token j at bits
// [2j, 2j+1] (oldest lowest), the forward window wants the newest token lowest.
DD_HD uint32_t pairrev32(uint32_t x) {
    x = __builtin_bitreverse32(x);  // v_bfrev_b32: fields reversed, but so are the two bits inside each
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}
DD_HD uint64_t pack64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// ---- a segment's token words, prepared once for the slices of its 64 tokens -----------------------------------------------
// Words 0..3 are the halo (the previous segment), 4..7 the segment.  A window is a slice of the token stream: behind token i
// of segment word w
//   the forward window's low word (newest token lowest) is  r[3+w]:r[4+w] >> (30 - 2 i),  r = the pair-reversed words;
//   the reverse-complement window's top word (stream order, newest on top) is  ~t[4+w]:~t[3+w] >> 2 (i + 1).
// The second count runs 2..32, and a funnel shift by 32 gives the older word: so d holds the complemented stream moved down
// by ONE token, d[n] = ~t[n+1]:~t[n] >> 2, and the slice is  d[4+w]:d[3+w] >> 2 i,  0..30 like the forward one.  (The two top
// bits of d[7] belong to the next segment: no slice reaches them.)  Every further word of a window is the same slice one
// word down.  A class that looks n words back uses the last n halo words only: the others are never computed.
struct SegWords {
    uint32_t r[8], d[8];
    DD_HD void fill(const uint4& hc, const uint4& sc) {
        const uint32_t t[8] = {hc.x, hc.y, hc.z, hc.w, sc.x, sc.y, sc.z, sc.w};
#pragma unroll
        for (int n = 0; n < 8; ++n) r[n] = pairrev32(t[n]);
#pragma unroll
        for (int n = 0; n < 7; ++n) d[n] = funnel32(~t[n + 1], ~t[n], 2);
        d[7] = ~t[7] >> 2;
    }
    // word j (0 = lowest) of the forward window, word j from the top of the reverse-complement window
    DD_HD uint32_t fwd(int w, int i, int j) const { return funnel32(r[3 + w - j], r[4 + w - j], 30u - 2u * (uint32_t)i); }
    DD_HD uint32_t rev(int w, int i, int j) const { return funnel32(d[4 + w - j], d[3 + w - j], 2u * (uint32_t)i); }
};

// ---- k-mer windows, one set per thread, shared by every k of the group --------------------------
// slice(sw, w, i): the windows behind token i of segment word w -- what 16 w + i + 1 pushes of (fw << 2) | c and
// (rc >> 2) | (3 - c) << top on the halo would leave -- cut from the prepared words, one funnel shift per 32-bit word
// (the count is wave-uniform: the walk's token loop is not unrolled).  tests/native/k1_windows.hip checks every form
// against those pushes on the host.
//   KC 0: k <= 16 (32-bit windows)   KC 1: 16 <= k <= 32 (64-bit)   KC 3: 33 <= k <= 48 (96-bit: 64 + 32)
//   KC 2: 49 <= k <= 64 (128-bit: Windows<7>, four 32-bit words)
template <int KC>
struct Windows;

template <>
struct Windows<0> {
    uint32_t fw = 0, rc = 0;
    DD_HD void slice(const SegWords& sw, int w, int i) {
        fw = sw.fwd(w, i, 0);
        rc = sw.rev(w, i, 0);
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {
        const uint32_t f = (k == 16) ? fw : (fw & ((1u << (2 * k)) - 1u));
        if (!CANON) return wang64_fast<true>(f);
        const uint32_t r = rc >> (32 - 2 * k);
        return wang64_fast<true>(f < r ? f : r);
    }
};

template <>
struct Windows<1> {
    uint64_t fw = 0, rc = 0;
    DD_HD void slice(const SegWords& sw, int w, int i) {
        fw = pack64(sw.fwd(w, i, 1), sw.fwd(w, i, 0));
        rc = pack64(sw.rev(w, i, 0), sw.rev(w, i, 1));
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {
        // 16 <= k <= 32: the low word of the window belongs to the k-mer whole, only the high word is masked
        const uint32_t mhi = (k == 32) ? ~0u : ((1u << (2 * k - 32)) - 1u);
        const uint64_t f = pack64((uint32_t)(fw >> 32) & mhi, (uint32_t)fw);
        if (!CANON) return wang64_fast<false>(f);
        const uint64_t r = rc >> (64 - 2 * k);
        return wang64_fast<false>(f < r ? f : r);
    }
};

// The 64-bit class again, as 32-bit halves: each is one slice, and the compiler has no 64-bit value to put together and
// take apart again.  Used by the scatter kernels, where the windows are cut per (token, k); sweep_kernel shares them between
// the ks of a group and keeps Windows<1> (measured equal there).
template <>
struct Windows<5> {
    uint32_t fl = 0, fh = 0, rl = 0, rh = 0;
    DD_HD void slice(const SegWords& sw, int w, int i) {
        fl = sw.fwd(w, i, 0);
        fh = sw.fwd(w, i, 1);
        rh = sw.rev(w, i, 0);
        rl = sw.rev(w, i, 1);
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {
        const uint32_t mhi = (k == 32) ? ~0u : ((1u << (2 * k - 32)) - 1u);
        const uint64_t f = pack64(fh & mhi, fl);
        if (!CANON) return wang64_fast<false>(f);
        const uint64_t r = pack64(rh, rl) >> (64 - 2 * k);
        return wang64_fast<false>(f < r ? f : r);
    }
};

// The tail the two 96-bit forms share: the hash of a k-mer of 66..96 bits, (hi, lo) with hi < 2^32 --
// fold128(hi, lo) as hi * G = hi * G_lo + ((hi * G_hi) << 32) (mod 2^64) -- and the canonical choice between the forward
// (ah, fl) and the reverse-complement (bh, bl) value in front of it.
DD_D uint64_t hash96(uint32_t hi, uint64_t lo) {
    const uint64_t hg = (uint64_t)hi * 0x7F4A7C15u + ((uint64_t)(hi * 0x9E3779B9u) << 32);
    return wang64_fast<false>(lo ^ hg);
}
DD_D uint64_t hash96_canonical(uint32_t ah, uint64_t fl, uint32_t bh, uint64_t bl) {
    const bool f_lt = (ah < bh) | ((ah == bh) & (fl < bl));  // bitwise: no exec-mask short circuit
    return hash96(f_lt ? ah : bh, f_lt ? fl : bl);
}

// 33 <= k <= 48: the k-mer is 66..96 bits, so the high part fits one 32-bit register and every
// step on it (mask, funnel shift of the reverse complement, compare, select, fold multiply) is a
// 32-bit instruction instead of a 64-bit pair.
template <>
struct Windows<3> {
    uint64_t fl = 0, rt = 0;  // forward: low 64 bits;  reverse complement, top-aligned: bits 95..32
    uint32_t fh = 0, rb = 0;  // forward: bits 95..64;  reverse complement: bits 31..0
    DD_HD void slice(const SegWords& sw, int w, int i) {
        fl = pack64(sw.fwd(w, i, 1), sw.fwd(w, i, 0));
        fh = sw.fwd(w, i, 2);
        rt = pack64(sw.rev(w, i, 0), sw.rev(w, i, 1));
        rb = sw.rev(w, i, 2);
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {
        const int hb = 2 * k - 64;  // 2..32 bits of the k-mer above bit 63
        const uint32_t ah = (hb == 32) ? fh : (fh & ((1u << hb) - 1u));
        if (!CANON) return hash96(ah, fl);
        const uint32_t s = 96u - 2u * (uint32_t)k;  // 0..30
        const uint32_t r3 = (uint32_t)(rt >> 32), r2 = (uint32_t)rt;
        return hash96_canonical(ah, fl, r3 >> s, pack64(__builtin_amdgcn_alignbit(r3, r2, s), __builtin_amdgcn_alignbit(r2, rb, s)));
    }
};

// The 96-bit class as three 32-bit words per window (see Windows<5>): used by the scatter kernels.
template <>
struct Windows<6> {
    uint32_t f0 = 0, f1 = 0, f2 = 0;  // forward window, low .. high word
    uint32_t r0 = 0, r1 = 0, r2 = 0;  // reverse complement, top-aligned in 96 bits: r2 holds bits 95..64
    DD_HD void slice(const SegWords& sw, int w, int i) {
        f0 = sw.fwd(w, i, 0);
        f1 = sw.fwd(w, i, 1);
        f2 = sw.fwd(w, i, 2);
        r2 = sw.rev(w, i, 0);
        r1 = sw.rev(w, i, 1);
        r0 = sw.rev(w, i, 2);
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {
        const int hb = 2 * k - 64;  // 2..32 bits of the k-mer above bit 63
        const uint32_t ah = (hb == 32) ? f2 : (f2 & ((1u << hb) - 1u));
        const uint64_t fl = pack64(f1, f0);
        if (!CANON) return hash96(ah, fl);
        const uint32_t s = 96u - 2u * (uint32_t)k;  // 0..30
        return hash96_canonical(ah, fl, r2 >> s, pack64(__builtin_amdgcn_alignbit(r2, r1, s), __builtin_amdgcn_alignbit(r1, r0, s)));
    }
};

// The 128-bit class as four 32-bit words per window (see Windows<5>): the one form of the class, for every kernel.
template <>
struct Windows<7> {
    uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;  // forward window, low .. high word
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;  // reverse complement, top-aligned in 128 bits
    DD_HD void slice(const SegWords& sw, int w, int i) {
        f0 = sw.fwd(w, i, 0);
        f1 = sw.fwd(w, i, 1);
        f2 = sw.fwd(w, i, 2);
        f3 = sw.fwd(w, i, 3);
        r3 = sw.rev(w, i, 0);
        r2 = sw.rev(w, i, 1);
        r1 = sw.rev(w, i, 2);
        r0 = sw.rev(w, i, 3);
    }
    template <bool CANON>
    DD_D uint64_t hash(int k) const {  // 49 <= k <= 64
        const int hb = 2 * k - 96;  // bits of the k-mer in the top word, 2..32
        const uint32_t mh = (hb == 32) ? ~0u : ((1u << hb) - 1u);
        const uint64_t ah = pack64(f3 & mh, f2);
        const uint64_t al = pack64(f1, f0);
        if (!CANON) return wang64_fast<false>(fold128(ah, al));
        const uint32_t s = 128u - 2u * (uint32_t)k;  // 0..30
        const uint64_t bh = pack64(r3 >> s, __builtin_amdgcn_alignbit(r3, r2, s));
        const uint64_t bl = pack64(__builtin_amdgcn_alignbit(r2, r1, s), __builtin_amdgcn_alignbit(r1, r0, s));
        const bool f_lt = (ah < bh) | ((ah == bh) & (al < bl));  // bitwise: no exec-mask short circuit
        return wang64_fast<false>(fold128(f_lt ? ah : bh, f_lt ? al : bl));
    }
};

// The form each kernel family uses for k class KC.  sweep_kernel: the 128-bit class as 32-bit words (Windows<7>: 1.6 % at
// log2m 16, 0.6 % at 14 on k 49..64); the 64- and 96-bit classes measure equal to slightly slower in that form there, where
// one push serves several ks, and keep u64 members.  The scatter kernels: 32-bit words for every class.
template <int KC>
using SweepWindows = Windows<KC == 2 ? 7 : KC>;
template <int KC>
using ScatterWindows = Windows<KC == 1 ? 5 : (KC == 3 ? 6 : (KC == 2 ? 7 : KC))>;

// a wave-uniform value that arrived through a vector load (a table entry): moved to scalar registers
DD_D uint64_t uniform64(uint64_t v) {
    // (the builtin returns int: without the casts the low half would be sign-extended over the high one)
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)), lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return ((uint64_t)hi << 32) | lo;
}
template <typename T>
DD_D T* uniform_ptr(T* q) { return reinterpret_cast<T*>(uniform64(reinterpret_cast<uint64_t>(q))); }

// ---- a tile's input and the walk over a segment (the hashed kernels) ---------------------------------------------------
// A thread's input for one tile: its segment (sc, sb) and the previous one (hc, hb: the halo the first windows reach into;
// segment 0 starts behind a BREAK).  A kernel issues the loads of tile t+1 before it processes tile t.  (fetch_tile fills
// the caller's TileIn: returning one by value changed the code around the loads, profiles/k1_shared_walk.txt.)
struct TileIn {
    uint4 hc, sc;
    uint2 hb, sb;
    bool live;  // the segment lies inside the token stream
};
DD_D void fetch_tile(const SweepGenome& g, const SweepJob& job, unsigned long long ntok, unsigned tile, TileIn& t) {
    const unsigned long long seg = (unsigned long long)tile * blockDim.x + threadIdx.x;
    t.live = tile < job.tile_end && seg * kSegTokens < ntok;
    t.hc = make_uint4(0, 0, 0, 0);
    t.hb = make_uint2(~0u, ~0u);
    t.sc = make_uint4(0, 0, 0, 0);  // a segment outside the stream is all BREAKs
    t.sb = make_uint2(~0u, ~0u);
    if (!t.live) return;
    if (seg > 0) {
        t.hc = gload16(g.codes + (seg - 1) * 4);
        t.hb = gload8(g.bad + (seg - 1) * 2);
    }
    t.sc = gload16(g.codes + seg * 4);
    t.sb = gload8(g.bad + seg * 2);
}

// The 64 tokens of a segment through the caller's windows `win` (cut here from the words of halo and segment, prepared once),
// reached by whole waves -- a segment outside the stream, or segment 0's halo, is zero codes behind BREAKs: its windows are cut
// like any other and never hashed into a register.  token(clean, run) is called behind every slice.  clean is std::true_type
// on the path where no lane of the wave has a BREAK within its halo or its segment (the common case away from record
// boundaries and N runs: every window of every k <= 64 is valid; run is not kept there and passed as 0), else std::false_type
// with run = the clean tokens that end at the current one.  (win is the caller's: the compiler's schedule of the token loops
// follows where it is declared, profiles/k1_shared_walk.txt.)
template <typename Win, typename Token>
DD_D void walk_segment(const TileIn& in, Win& win, const Token& token) {
    const uint2 hb = in.hb, sb = in.sb;
    SegWords sw;
    sw.fill(in.hc, in.sc);
    if (__all((hb.x | hb.y | sb.x | sb.y) == 0u)) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
#pragma unroll 1
            for (int i = 0; i < 16; ++i) {
                win.slice(sw, w, i);
                token(std::true_type{}, 0);
            }
        }
        return;
    }
    // run enters as the clean tail of the halo
    int run = hb.y ? __builtin_clz(hb.y) : 32 + (hb.x ? __builtin_clz(hb.x) : 32);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t bw = ((w & 2) ? sb.y : sb.x) >> ((w & 1) * 16);
#pragma unroll 1
        for (int i = 0; i < 16; ++i) {
            run = ((bw >> i) & 1u) ? 0 : run + 1;
            win.slice(sw, w, i);
            token(std::false_type{}, run);
        }
    }
}

// ---- the small-k classes' segment (bitmap_kernel, bigmap_kernel) -------------------------------------------------------
// One 32-bit window pair.  WHOLE (bitmap_kernel): the newest 16 tokens, every k masks its own k-mer out; else (bigmap_kernel)
// cut to the job's one k: mask = 4^k - 1, top = 2 k - 2.
template <bool WHOLE>
struct SmallWindows {
    uint32_t mask;
    int top;
    uint32_t fw = 0, rc = 0;
    DD_D void push(uint32_t c) {
        fw = WHOLE ? (fw << 2) | c : ((fw << 2) | c) & mask;
        rc = (rc >> 2) | ((3u - c) << (WHOLE ? 30 : top));
    }
};
// A thread's segment, the windows primed from the last `prime` tokens of the halo (prime <= 10: its last code word), and
// run = the clean tokens that end the halo, among those
struct SmallIn {
    uint4 sc;
    uint2 sb;
    int run;
};
template <typename Win>
DD_D SmallIn fetch_small(const SweepGenome& g, unsigned long long seg, int prime, Win& win) {
    SmallIn s;
    s.run = 0;
    if (seg > 0) {
        const uint4 hc = gload16(g.codes + (seg - 1) * 4);
        const uint2 hb = gload8(g.bad + (seg - 1) * 2);
        const uint32_t cw = hc.w, bw = hb.y >> 16;
#pragma unroll 1
        for (int i = 16 - prime; i < 16; ++i) {
            const uint32_t c = (cw >> (2 * i)) & 3u;
            s.run = ((bw >> i) & 1u) ? 0 : s.run + 1;
            win.push(c);
        }
    }
    s.sc = gload16(g.codes + seg * 4);
    s.sb = gload8(g.bad + seg * 2);
    return s;
}

// ---- exact k-mer sets -> registers (bitmap_finish_kernel, bigmap_finish_kernel) and records -> registers (replay_kernel) --
// LDS register a = max(., rho)
DD_D void lds_raise(uint32_t a, uint32_t rho) {
    const uint32_t w = RegsLds::load32(a);
    if (rho > ((w >> RegsLds::shift(a)) & 0xFFu)) (void)cas_raise<RegsLds>(a, w, rho);
}
// f(32 w + bit) for every set bit of the nw words at bm, the words dealt round the workgroup
template <typename F>
DD_D void for_each_set_bit(const uint32_t* bm, uint32_t nw, const F& f) {
    for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) {
        uint32_t v = gload4(bm + w);
        while (v) {
            const uint32_t bit = (uint32_t)__builtin_ctz(v);
            v &= v - 1;
            f((w << 5) | bit);
        }
    }
}
// Index tile b (2^tile_log2 registers, at `out`) of a row built in LDS from ALL the k-mers of its set: for_each_kmer(emit)
// calls emit(x) for every k-mer x (< 2^32) the workgroup's threads find; those whose register lies in another tile are dropped.
template <typename ForEachKmer>
DD_D void finish_tile(uint8_t* out, int tile_log2, uint32_t b, int p, const ForEachKmer& for_each_kmer) {
    const uint32_t tile = 1u << tile_log2;
    uint4* z = reinterpret_cast<uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < (tile >> 4); i += blockDim.x) z[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for_each_kmer([&](uint32_t x) {
        const Probe q = probe(wang64_fast<true>(x), p);
        const uint32_t idx = q.hi >> (32 - p);
        if ((idx >> tile_log2) != b) return;
        lds_raise(idx & (tile - 1u), rho_of(q, p));
    });
    __syncthreads();
    const uint4* l4 = reinterpret_cast<const uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < (tile >> 4); i += blockDim.x) gstore16(out + (size_t)i * 16, l4[i]);
}

// ---- host: pick the instantiation, launch it -----------------------------------------------------------------------------
// f(std::integral_constant<int, KC>, std::bool_constant<CANON>) for the k class and strand mode of a launch
template <typename F>
void dispatch_kc_canon(int kclass, bool canonical, const F& f) {
    dispatch_bool(canonical, [&](auto cn) {
        if (kclass == 0) f(std::integral_constant<int, 0>{}, cn);
        else if (kclass == 1) f(std::integral_constant<int, 1>{}, cn);
        else if (kclass == 3) f(std::integral_constant<int, 3>{}, cn);
        else f(std::integral_constant<int, 2>{}, cn);
    });
}

}  // namespace dd
