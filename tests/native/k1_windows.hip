// k1_windows.hip -- the window slices of dd_k1.h (SegWords, Windows<...>::slice) against plain pushes, on the host.
// A stand-alone program: only the host side of the source is compiled, nothing touches a GPU.
//   hipcc --offload-host-only -std=c++17 -O1 -Idandd_amd/csrc tests/native/k1_windows.hip -o k1_windows
//   (add -Xarch_host -fsanitize=address,undefined to run it under the sanitizers: host code only)
// For every window form: random and edge words (all zero, all ones, alternating), every word and token position
// (w = 0..3, i = 0..15), against 16 w + i + 1 pushes of the segment's tokens onto windows that hold the halo's 64; for every
// k of the form's class the k-mer the hash would read out of the sliced members -- forward value, reverse-complement value --
// against the k-mer read straight from the tokens.  And the funnel shift's count: 32 gives the low word.
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

// 128-bit windows as four words, word 0 lowest, pushed one token at a time: the definition the slices stand for
struct Pushed {
    uint32_t f[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    void push(uint32_t c) {
        for (int j = 3; j > 0; --j) f[j] = (f[j] << 2) | (f[j - 1] >> 30);
        f[0] = (f[0] << 2) | c;
        for (int j = 0; j < 3; ++j) r[j] = (r[j] >> 2) | (r[j + 1] << 30);
        r[3] = (r[3] >> 2) | ((3u - c) << 30);
    }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd32() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// the forward words low .. high and the reverse-complement words top .. down of each form, as the hash reads them
void words_of(const Windows<0>& v, uint32_t* f, uint32_t* r) { f[0] = v.fw, r[0] = v.rc; }
void words_of(const Windows<1>& v, uint32_t* f, uint32_t* r) {
    f[0] = (uint32_t)v.fw, f[1] = (uint32_t)(v.fw >> 32), r[0] = (uint32_t)(v.rc >> 32), r[1] = (uint32_t)v.rc;
}
void words_of(const Windows<5>& v, uint32_t* f, uint32_t* r) { f[0] = v.fl, f[1] = v.fh, r[0] = v.rh, r[1] = v.rl; }
void words_of(const Windows<3>& v, uint32_t* f, uint32_t* r) {
    f[0] = (uint32_t)v.fl, f[1] = (uint32_t)(v.fl >> 32), f[2] = v.fh, r[0] = (uint32_t)(v.rt >> 32), r[1] = (uint32_t)v.rt, r[2] = v.rb;
}
void words_of(const Windows<6>& v, uint32_t* f, uint32_t* r) { f[0] = v.f0, f[1] = v.f1, f[2] = v.f2, r[0] = v.r2, r[1] = v.r1, r[2] = v.r0; }
void words_of(const Windows<7>& v, uint32_t* f, uint32_t* r) {
    f[0] = v.f0, f[1] = v.f1, f[2] = v.f2, f[3] = v.f3, r[0] = v.r3, r[1] = v.r2, r[2] = v.r1, r[3] = v.r0;
}

// bit b of a value held as NW words, word 0 lowest
uint32_t bit_of(const uint32_t* v, int nw, int b) { return b < 32 * nw ? (v[b >> 5] >> (b & 31)) & 1u : 0u; }

// One input (halo words hc, segment words sc) through form FORM of NW words per window, ks kmin..kmax.
template <int FORM, int NW>
void check_form(const uint32_t* hc, const uint32_t* sc, int kmin, int kmax, const char* what) {
    SegWords sw;
    sw.fill(make_uint4(hc[0], hc[1], hc[2], hc[3]), make_uint4(sc[0], sc[1], sc[2], sc[3]));
    Pushed ref;
    uint32_t tok[128];
    for (int t = 0; t < 64; ++t) tok[t] = (hc[t >> 4] >> (2 * (t & 15))) & 3u;
    for (int t = 0; t < 64; ++t) tok[64 + t] = (sc[t >> 4] >> (2 * (t & 15))) & 3u;
    for (int t = 0; t < 64; ++t) ref.push(tok[t]);  // the 64 pushes from the halo
    for (int w = 0; w < 4; ++w) {
        for (int i = 0; i < 16; ++i) {
            ref.push(tok[64 + 16 * w + i]);
            Windows<FORM> win;
            win.slice(sw, w, i);
            uint32_t f[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
            words_of(win, f, r);
            for (int j = 0; j < NW; ++j) {
                CHECK(f[j] == ref.f[j], "%s form %d w %d i %d: forward word %d is %08x, pushes give %08x", what, FORM, w, i, j, f[j], ref.f[j]);
                CHECK(r[j] == ref.r[3 - j], "%s form %d w %d i %d: reverse word %d from the top is %08x, pushes give %08x", what,
                      FORM, w, i, j, r[j], ref.r[3 - j]);
            }
            // every k of the class: the k-mer itself, token by token
            const int last = 64 + 16 * w + i;
            uint32_t rlow[4];  // the reverse-complement window as a value, word 0 lowest
            for (int j = 0; j < NW; ++j) rlow[j] = r[NW - 1 - j];
            for (int k = kmin; k <= kmax; ++k) {
                for (int q = 0; q < k; ++q) {
                    // forward: the newest token lowest; reverse complement: the complement of the newest token highest of 2 k bits
                    const uint32_t c = tok[last - q];
                    const uint32_t fq = bit_of(f, NW, 2 * q) | (bit_of(f, NW, 2 * q + 1) << 1);
                    const int at = 32 * NW - 2 * k + 2 * (k - 1 - q);
                    const uint32_t rq = bit_of(rlow, NW, at) | (bit_of(rlow, NW, at + 1) << 1);
                    CHECK(fq == c, "%s form %d w %d i %d k %d: forward token %d back is %u, stream has %u", what, FORM, w, i, k, q, fq, c);
                    CHECK(rq == 3u - c, "%s form %d w %d i %d k %d: reverse token %d back is %u, stream has %u", what, FORM, w, i, k, q, rq, 3u - c);
                }
            }
        }
    }
}

void check_input(const uint32_t* hc, const uint32_t* sc, const char* what) {
    check_form<0, 1>(hc, sc, 1, 16, what);
    check_form<1, 2>(hc, sc, 16, 32, what);
    check_form<5, 2>(hc, sc, 16, 32, what);
    check_form<3, 3>(hc, sc, 33, 48, what);
    check_form<6, 3>(hc, sc, 33, 48, what);
    check_form<7, 4>(hc, sc, 49, 64, what);
}

}  // namespace

int main() {
    // the funnel shift as the device instruction takes its count: modulo 32
    CHECK(funnel32(0xAAAAAAAAu, 0x55555555u, 0) == 0x55555555u, "funnel32 count 0");
    CHECK(funnel32(0xAAAAAAAAu, 0x55555555u, 32) == 0x55555555u, "funnel32 count 32 gives the LOW word");
    CHECK(funnel32(0x00000001u, 0x80000000u, 31) == 0x00000003u, "funnel32 count 31");
    CHECK(funnel32(0x12345678u, 0x9ABCDEF0u, 8) == 0x789ABCDEu, "funnel32 count 8");
    CHECK(pairrev32(0x0000001Bu) == 0xE4000000u, "pairrev32");

    const uint32_t edge[4] = {0u, ~0u, 0xAAAAAAAAu, 0x1B1B1B1Bu};
    uint32_t hc[4], sc[4];
    // edge words: all of one kind, and each kind in the halo against each in the segment
    for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b) {
            for (int j = 0; j < 4; ++j) hc[j] = edge[a], sc[j] = edge[b];
            check_input(hc, sc, "edge");
        }
    }
    // one edge word among random ones, at every place
    for (int at = 0; at < 8; ++at) {
        for (int e = 0; e < 2; ++e) {
            for (int j = 0; j < 4; ++j) hc[j] = rnd32(), sc[j] = rnd32();
            (at < 4 ? hc[at] : sc[at - 4]) = edge[e];
            check_input(hc, sc, "edge among random");
        }
    }
    for (int n = 0; n < 200; ++n) {
        for (int j = 0; j < 4; ++j) hc[j] = rnd32(), sc[j] = rnd32();
        check_input(hc, sc, "random");
    }
    if (g_fail) {
        printf("k1_windows: %d checks FAILED\n", g_fail);
        return 1;
    }
    printf("k1_windows: ok (%lld comparisons)\n", g_checks);
    return 0;
}
