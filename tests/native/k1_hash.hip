// k1_hash.hip -- the K1 hash and register probe of dd_k1.h (mul64_c32, mul64_c32_fold, wang64_fast, probe, RegsLds::at) against
// their definitions, on the host.  A stand-alone program: only the host side of the source is compiled, nothing touches a GPU.
//   hipcc --offload-host-only -std=c++17 -O1 -Idandd_amd/csrc tests/native/k1_hash.hip -o k1_hash
//   (add -Xarch_host -fsanitize=address,undefined to run it under the sanitizers: host code only)
// The host forms are plain C where the device has an instruction, but the ARRANGEMENT is shared: the multiply by 265 as
// lo * C + (mul_lo(hi, C) << 32), the first multiply as a mad plus a separate high product, the probe as funnel shifts.
// Hash: wang64_fast<false>(x) and wang64_fast<true>(x32) against dd::wang64 on every pair of edge words, on the keys whose
// value ENTERING the multiply by 265 is each such pair (made by running the first two steps backwards: they include the
// largest carry out of lo * 265 and hi = 0xFFFFFFFF), and on seeded random values.
// Probe: for every p = 4 .. 16, every slot whose registers lie within 160 KiB, and edge and random hashes: the register's LDS
// address (slot << p) | (h >> (64 - p)), the 32 bits behind the index, and the leading-zero count including that of zero.
#include "dd_k1.h"

#include <stdio.h>

using namespace dd;

namespace {

int g_fail = 0;
long long g_checks = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checks;                                        \
        if (!(cond)) {                                     \
            if (g_fail++ < 20) {                           \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd64() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

const uint32_t kEdge[6] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0x00F0F0F1u};

// the inverse of an odd c modulo 2^64 (Newton: every step doubles the correct low bits, 3 -> 96 in five)
uint64_t inverse(uint64_t c) {
    uint64_t x = c;  // correct to 3 bits: c * c == 1 (mod 8)
    for (int i = 0; i < 5; ++i) x *= 2 - c * x;
    return x;
}
// the x with x ^ (x >> s) == y
uint64_t unxorshift(uint64_t y, int s) {
    for (int t = s; t < 64; t *= 2) y ^= y >> t;
    return y;
}
// the key whose value entering the multiply by 265 is y: the first two steps of the mix, backwards
uint64_t key_before_265(uint64_t y) { return (unxorshift(y, 24) + 1) * inverse(0x1FFFFFull); }

// leading zeros of x by looking at every bit; 0xFFFFFFFF for zero, as v_ffbh_u32
uint32_t leading_zeros(uint32_t x) {
    if (!x) return ~0u;
    uint32_t n = 0;
    while (!((x >> (31 - n)) & 1u)) ++n;
    return n;
}

void check_hash(uint64_t x, const char* what) {
    const uint64_t want = wang64(x), got = wang64_fast<false>(x);
    CHECK(got == want, "%s: wang64_fast<false>(%016llx) is %016llx, wang64 gives %016llx", what, (unsigned long long)x,
          (unsigned long long)got, (unsigned long long)want);
    const uint32_t x32 = (uint32_t)x;
    const uint64_t want32 = wang64(x32), got32 = wang64_fast<true>(x32);
    CHECK(got32 == want32, "%s: wang64_fast<true>(%08x) is %016llx, wang64 gives %016llx", what, x32, (unsigned long long)got32,
          (unsigned long long)want32);
}

void check_probe(uint64_t h, int p, uint32_t slot, const char* what) {
    const Probe q = probe(h, p);
    const uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
    const uint32_t a = RegsLds{slot}.at(q.hi, p);
    CHECK(a == ((slot << p) | (uint32_t)(h >> (64 - p))), "%s p %d slot %u h %016llx: address %08x", what, p, slot, (unsigned long long)h, a);
    CHECK(a >= (slot << p) && a < ((slot + 1u) << p) && a < 160u * 1024u, "%s p %d slot %u: address %08x outside the slot's registers", what, p, slot, a);
    CHECK(q.hiw == (uint32_t)((h << p) >> 32), "%s p %d h %016llx: hiw %08x", what, p, (unsigned long long)h, q.hiw);
    CHECK(q.lz == leading_zeros(q.hiw), "%s p %d h %016llx: lz %08x of hiw %08x", what, p, (unsigned long long)h, q.lz, q.hiw);
    CHECK(q.lo == lo && q.hi == hi, "%s p %d h %016llx: words %08x %08x", what, p, (unsigned long long)h, q.hi, q.lo);
}

}  // namespace

int main() {
    CHECK(inverse(0x1FFFFFull) * 0x1FFFFFull == 1ull && inverse(265) * 265ull == 1ull, "inverse");
    CHECK(ffbh(0u) == ~0u && ffbh(1u) == 31u && ffbh(0x80000000u) == 0u, "ffbh");

    // ---- the hash ----
    long long max_carry = 0;
    bool saw_hi_ones = false;
    for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) {
            const uint64_t w = pack64(kEdge[a], kEdge[b]);
            check_hash(w, "edge pair");
            // the two multiplies on the pair itself
            CHECK(mul64_c32_fold(w, 265u) == w * 265ull, "mul64_c32_fold(%016llx, 265)", (unsigned long long)w);
            CHECK(mul64_c32<false>(w, 0x1FFFFFu, ~0ull) == ~w + (w << 21), "mul64_c32<false>(%016llx, 2^21 - 1, -1)", (unsigned long long)w);
            CHECK(mul64_c32<true>(kEdge[b], 0x1FFFFFu, ~0ull) == ~(uint64_t)kEdge[b] + ((uint64_t)kEdge[b] << 21), "mul64_c32<true>(%08x, 2^21 - 1, -1)", kEdge[b]);
            // the key that brings the pair to the multiply by 265
            const uint64_t x = key_before_265(w);
            uint64_t y = mul64_c32<false>(x, 0x1FFFFFu, ~0ull);
            y ^= y >> 24;
            CHECK(y == w, "key %016llx enters the multiply by 265 as %016llx, not %016llx", (unsigned long long)x, (unsigned long long)y, (unsigned long long)w);
            check_hash(x, "preimage");
            const long long carry = (long long)(((uint64_t)kEdge[b] * 265ull) >> 32);
            max_carry = carry > max_carry ? carry : max_carry;
            saw_hi_ones |= kEdge[a] == 0xFFFFFFFFu && carry == 264;
        }
    }
    CHECK(max_carry == 264 && saw_hi_ones, "the edge pairs reach carry %lld out of lo * 265 (264 is the largest there is)", max_carry);
    for (int n = 0; n < 1200000; ++n) check_hash(rnd64(), "random");
    for (int n = 0; n < 100000; ++n) check_hash(rnd64() >> (n & 63), "random, short");  // (few significant bits: small k)

    // ---- the probe ----
    for (int p = 4; p <= 16; ++p) {
        uint64_t hs[96];
        int nh = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) hs[nh++] = pack64(kEdge[a], kEdge[b]);
        const int q = 64 - p;
        hs[nh++] = ((1ull << p) - 1ull) << q;                  // the last register, everything behind the index zero
        hs[nh++] = (((1ull << p) - 1ull) << q) | ((1ull << (q - 32)) - 1ull);  // ... hiw == 0, every bit behind it set
        hs[nh++] = 1ull << (q - 32);                           // hiw == 1
        hs[nh++] = (1ull << (q - 32)) - 1ull;                  // hiw == 0, lo != 0
        hs[nh++] = 1ull << (q - 1);                            // hiw's top bit: lz == 0
        hs[nh++] = (1ull << q) - 1ull;                         // register 0, hiw all ones
        hs[nh++] = 1ull << q;                                  // register 1, hiw == 0
        for (int n = 0; n < 16; ++n) hs[nh++] = rnd64();
        for (int n = 0; n < 8; ++n) hs[nh++] = rnd64() & ~(0xFFFFFFFFull << (q - 32));  // random index, hiw == 0
        const uint32_t nslots = (160u * 1024u) >> p;           // (slot + 1) << p <= 160 KiB
        for (uint32_t slot = 0; slot < nslots; ++slot)
            for (int n = 0; n < nh; ++n) check_probe(hs[n], p, slot, "probe");
    }
    if (g_fail) {
        printf("k1_hash: %d checks FAILED\n", g_fail);
        return 1;
    }
    printf("k1_hash: ok (%lld comparisons)\n", g_checks);
    return 0;
}
