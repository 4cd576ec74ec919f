"""Generates tests/golden/rare_rho.json: k-mers of k <= 31 whose HLL update has rho >= 33 (tests/rare_rho.py says why
they are wanted).  For k <= 31 the key wang64 is applied to must have its top 64 - 2k bits zero, so such k-mers have to
be searched for:

  k <= 17   every key below 4^17 is hashed FORWARDS once (2^34 hashes) and checked at every log2m 4..20.  That is
            exhaustive: the fixture holds EVERY k-mer of k <= 16 with rho >= 33 at every log2m 4..20 ("counts" says how
            many there are for every k <= 17, the zeros included: none for any k <= 12 at any log2m; a key below 4^k
            is a k-mer for every longer k too, with As in front), and for k = 17 up to 8 per log2m of LOG2M and at log2m 4.
  k = 20, 24, 28, 31   for every log2m of LOG2M all 2^32 hashes  idx << q | tail  whose 32 bits behind the index are zero
            are inverted (tests/rare_rho.py: inv_wang64, restated in C below and checked against the Python form
            here); a key below 4^k is a hit.  Up to 8 are kept per (k, log2m): of rho 33, 34, the largest found, then
            downwards from there, in turn, at distinct register indices, usable in canonical mode and not alternately.

The scans run in a small C program compiled into a temporary directory (cc -O2 -pthread; about 8 CPU-minutes in all);
what it reports is checked entry by entry with tests/pyref.py before it is written.  Nothing from oracle/ or
dandd_amd/ is used.  Run from the repo root:  python tests/golden/make_rare_rho.py"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pyref  # noqa: E402
import rare_rho  # noqa: E402

LOG2M = [10, 14, 16, 17, 18, 20]     # for k = 17 .. 31
KS_INVERSE = [20, 24, 28, 31]
PER_PAIR = 8
KEEP = 4                             # the scan keeps the first KEEP hits (in scan order) per (k, log2m, rho, canonical or not)

C_SOURCE = r"""
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NT 8
#define KEEP 4
typedef uint64_t u64;

static u64 wang64(u64 key) {
    key = ~key + (key << 21);
    key ^= key >> 24;
    key = key + (key << 3) + (key << 8);
    key ^= key >> 14;
    key = key + (key << 2) + (key << 4);
    key ^= key >> 28;
    return key + (key << 31);
}
static u64 inv_odd(u64 c) {  /* Newton: c is its own inverse mod 8, every step doubles the correct bits */
    u64 x = c;
    for (int i = 0; i < 6; ++i) x *= 2 - c * x;
    return x;
}
static u64 I1, I2, I3, I4;
static u64 inv_wang64(u64 x) {
    x *= I4;
    x ^= x >> 28; x ^= x >> 56;
    x *= I3;
    x ^= x >> 14; x ^= x >> 28; x ^= x >> 56;
    x *= I2;
    x ^= x >> 24; x ^= x >> 48;
    return (x + 1) * I1;
}
static int rho_of(u64 h, int p) {
    const int q = 64 - p;
    const u64 tail = h & ((1ull << q) - 1);
    return tail ? __builtin_clzll(tail) - p + 1 : q + 1;
}
static int canonical(u64 x, int k) {
    u64 f = x, rc = 0;
    for (int i = 0; i < k; ++i) { rc = (rc << 2) | (3 - (f & 3)); f >>= 2; }
    return x <= rc;
}

/* forward: every key in [lo, hi) */
typedef struct { u64 lo, hi; u64 *hits; size_t n, cap; } Fwd;
static void *fwd_run(void *arg) {
    Fwd *w = arg;
    for (u64 x = w->lo; x < w->hi; ++x) {
        const u64 h = wang64(x);
        if ((h >> 28) & 0xFFFF) continue;   /* bits 43..28 are behind the index at every log2m 4..20 */
        for (int p = 4; p <= 20; ++p)
            if ((uint32_t)((h << p) >> 32) == 0) {
                if (w->n == w->cap) w->hits = realloc(w->hits, (w->cap *= 2) * 2 * sizeof(u64));
                w->hits[2 * w->n] = x;
                w->hits[2 * w->n + 1] = (u64)p;
                ++w->n;
            }
    }
    return 0;
}

/* inverse: counters [lo, hi) of 2^32 at one log2m; counter = tail << p | idx */
#define NK 4
static const int KS[NK] = {20, 24, 28, 31};
typedef struct { u64 lo, hi; int p; u64 count[NK]; u64 keep[NK][64][2][KEEP]; int nkeep[NK][64][2]; } Inv;
static void *inv_run(void *arg) {
    Inv *w = arg;
    const int p = w->p, q = 64 - p;
    for (u64 c = w->lo; c < w->hi; ++c) {
        const u64 h = ((c & ((1ull << p) - 1)) << q) | (c >> p);
        const u64 x = inv_wang64(h);
        if (x >> 62) continue;
        const int rho = rho_of(h, p);
        for (int j = 0; j < NK; ++j) {
            if (x >> (2 * KS[j])) continue;
            ++w->count[j];
            if (w->nkeep[j][rho][0] == KEEP && w->nkeep[j][rho][1] == KEEP) continue;
            const int cn = canonical(x, KS[j]);
            if (w->nkeep[j][rho][cn] < KEEP) w->keep[j][rho][cn][w->nkeep[j][rho][cn]++] = x;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    I1 = inv_odd((1ull << 21) - 1); I2 = inv_odd(265); I3 = inv_odd(21); I4 = inv_odd((1ull << 31) + 1);
    for (u64 x = 0; x < 100000; ++x)
        if (inv_wang64(wang64(x * 0x9E3779B97F4A7C15ull)) != x * 0x9E3779B97F4A7C15ull) return 2;
    pthread_t th[NT];
    if (argc == 3 && !strcmp(argv[1], "forward")) {
        const u64 n = 1ull << (2 * atoi(argv[2]));
        static Fwd w[NT];
        for (int t = 0; t < NT; ++t) {
            w[t].lo = n / NT * t; w[t].hi = t == NT - 1 ? n : n / NT * (t + 1);
            w[t].cap = 64; w[t].n = 0; w[t].hits = malloc(w[t].cap * 2 * sizeof(u64));
            pthread_create(&th[t], 0, fwd_run, &w[t]);
        }
        for (int t = 0; t < NT; ++t) {
            pthread_join(th[t], 0);
            for (size_t i = 0; i < w[t].n; ++i) {
                const u64 x = w[t].hits[2 * i]; const int p = (int)w[t].hits[2 * i + 1];
                printf("F %llu %d %llu %d\n", (unsigned long long)x, p, (unsigned long long)(wang64(x) >> (64 - p)), rho_of(wang64(x), p));
            }
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "inverse")) {
        static Inv w[NT];
        const u64 n = 1ull << 32;
        for (int t = 0; t < NT; ++t) {
            memset(&w[t], 0, sizeof w[t]);
            w[t].p = atoi(argv[2]); w[t].lo = n / NT * t; w[t].hi = n / NT * (t + 1);
            pthread_create(&th[t], 0, inv_run, &w[t]);
        }
        for (int t = 0; t < NT; ++t) pthread_join(th[t], 0);
        for (int j = 0; j < NK; ++j) {
            u64 count = 0;
            for (int t = 0; t < NT; ++t) count += w[t].count[j];
            printf("C %d %llu\n", KS[j], (unsigned long long)count);
            for (int rho = 0; rho < 64; ++rho)
                for (int cn = 0; cn < 2; ++cn) {
                    int got = 0;   /* the first KEEP in counter order, whatever the number of threads */
                    for (int t = 0; t < NT; ++t)
                        for (int i = 0; i < w[t].nkeep[j][rho][cn] && got < KEEP; ++i, ++got)
                            printf("B %d %d %d %llu\n", KS[j], rho, cn, (unsigned long long)w[t].keep[j][rho][cn][i]);
                }
        }
        return 0;
    }
    return 1;
}
"""


def check_inverse():
    rnd = random.Random(20261018)
    for x in [0, 2**64 - 1] + [rnd.getrandbits(64) for _ in range(2000)]:
        assert rare_rho.inv_wang64(pyref.wang64(x)) == x, hex(x)
        assert pyref.wang64(rare_rho.inv_wang64(x)) == x, hex(x)


def entry(k, p, x):
    """[k, log2m, k-mer, usable in canonical mode, idx, rho], everything recomputed with pyref"""
    s = rare_rho.kmer_str(x, k)
    assert rare_rho.kmer_int(s) == x and x < 4**k
    idx, rho = pyref.idx_rho(pyref.wang64(x), p)
    assert rho >= 33, (k, p, s, rho)
    return [k, p, s, rare_rho.is_canonical(s), idx, rho]


def pick(cands):
    """cands: entries of one (k, log2m) in scan order -> up to PER_PAIR of them: rho 33, 34, the largest, then downwards
    from the largest, one at a time round and round; in each round the canonical flag wanted alternates; distinct indices."""
    rhos = sorted({e[5] for e in cands})
    order = [r for r in (33, 34, rhos[-1]) if r in rhos]
    order = list(dict.fromkeys(order + rhos[::-1]))
    out, seen_idx, rnd = [], set(), 0
    left = list(cands)
    while len(out) < PER_PAIR and left:
        took = False
        for j, rho in enumerate(order):
            want_canon = (rnd + j) % 2 == 0
            pool = [e for e in left if e[5] == rho and e[4] not in seen_idx]
            pool.sort(key=lambda e: e[3] != want_canon)      # stable: scan order within a flag
            if pool and len(out) < PER_PAIR:
                out.append(pool[0])
                seen_idx.add(pool[0][4])
                left.remove(pool[0])
                took = True
        if not took:
            break
        rnd += 1
    return out


def main():
    check_inverse()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "scan.c"), os.path.join(tmp, "scan")
        with open(src, "w") as f:
            f.write(C_SOURCE)
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-pthread", "-o", exe, src])
        fwd = subprocess.check_output([exe, "forward", "17"], text=True).split("\n")
        inv = {p: subprocess.check_output([exe, "inverse", str(p)], text=True).split("\n") for p in LOG2M}

    counts, entries = {}, []
    hits = sorted((int(p), int(x), int(idx), int(rho)) for _, x, p, idx, rho in (l.split() for l in fwd if l))
    for p, x, idx, rho in hits:
        assert pyref.idx_rho(pyref.wang64(x), p) == (idx, rho)
    for k in range(1, 18):
        counts[str(k)] = {str(p): sum(1 for pp, x, _, _ in hits if pp == p and x < 4**k) for p in range(4, 21)}
    for k in range(1, 17):
        for p in range(4, 21):
            entries += [entry(k, p, x) for pp, x, _, _ in hits if pp == p and x < 4**k]
    for p in [4] + LOG2M:            # (the forward scan has every log2m: 4 as well, the one with the largest rho)
        entries += pick([entry(17, p, x) for pp, x, _, _ in hits if pp == p])
    for k in KS_INVERSE:
        counts[str(k)] = {}
        for p in LOG2M:
            rows = [l.split() for l in inv[p] if l]
            counts[str(k)][str(p)] = next(int(r[2]) for r in rows if r[0] == "C" and int(r[1]) == k)
            entries += pick([entry(k, p, int(r[4])) for r in rows if r[0] == "B" and int(r[1]) == k])
    out = {"counts": counts, "entries": entries}
    with open(os.path.join(HERE, "rare_rho.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("wrote rare_rho.json:", len(entries), "entries")
    for k in ("13", "14", "15", "16", "17"):
        print("k", k, counts[k])


if __name__ == "__main__":
    main()
