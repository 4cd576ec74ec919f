"""k-mers whose HLL update has rho >= 33 (the 32 hash bits behind the register index all zero: one hash in 2^32), made on
purpose.  Wang's 64-bit mix is a bijection, so any wanted hash  idx << q | tail  has a key (inv_wang64), and a key is a
k-mer: the 32-mer itself, for k >= 33 any high part with the low word solved through fold128, and for k <= 31 only where
the key's top 64 - 2k bits happen to be zero (searched once, tests/golden/make_rare_rho.py -> tests/golden/rare_rho.json).
Plain Python ints; nothing from oracle/ or the product.  Used by tests/test_rare_rho.py (CPU: pins the oracle with pyref on
these inputs) and tests/test_gpu_rare_rho.py (every K1 family against the oracle)."""
import json
import os
import random

import pyref

M64 = pyref.M64
G = 0x9E3779B97F4A7C15                     # fold128's multiplier (pyref.fold128)
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "rare_rho.json")


def _unxorshift(x, s):
    """the x with x ^ (x >> s) == the argument"""
    t = s
    while t < 64:
        x ^= x >> t
        t *= 2
    return x


_INV_2P21M1 = pow((1 << 21) - 1, -1, 1 << 64)
_INV_265 = pow(265, -1, 1 << 64)
_INV_21 = pow(21, -1, 1 << 64)
_INV_2P31P1 = pow((1 << 31) + 1, -1, 1 << 64)


def inv_wang64(h):
    """pyref.wang64 backwards, step by step: the multiplications by odd constants through their inverses mod 2^64, the
    xor-shifts by iteration, the first step as  x (2^21 - 1) - 1."""
    x = (h * _INV_2P31P1) & M64            # key + (key << 31)
    x = _unxorshift(x, 28)
    x = (x * _INV_21) & M64                # key + (key << 2) + (key << 4)
    x = _unxorshift(x, 14)
    x = (x * _INV_265) & M64               # key + (key << 3) + (key << 8)
    x = _unxorshift(x, 24)
    return ((x + 1) * _INV_2P21M1) & M64   # ~key + (key << 21)


def kmer_str(x, k):
    return "".join("ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_int(s):
    x = 0
    for c in s:
        x = (x << 2) | "ACGT".index(c)
    return x


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def is_canonical(s):
    """the k-mer is the one a canonical sketch hashes (<= its reverse complement as a 2k-bit number: A < C < G < T)"""
    return s <= revcomp(s)


def key_of(s):
    """what wang64 is applied to for the k-mer s (NOT canonicalised)"""
    x = kmer_int(s)
    return x if len(s) <= 32 else pyref.fold128(x >> 64, x & M64)


def idx_rho_of(s, p):
    return pyref.idx_rho(pyref.wang64(key_of(s)), p)


def rho_targets(p):
    """31 and 32: the last values of the short form (the 32 bits behind the index are 2 or 3, and 1); 33, 34, 40; q - 1, q, and
    q + 1 (an all-zero tail: the largest value a register of 2^p can hold)"""
    q = 64 - p
    return [31, 32, 33, 34, 40, q - 1, q, q + 1]


def target_hash(idx, rho, p, rng):
    """a hash with register index idx and exactly rho; the tail bits behind the leading one are random"""
    q = 64 - p
    assert 0 <= idx < (1 << p) and 1 <= rho <= q + 1
    if rho == q + 1:
        return idx << q
    free = q - rho
    return (idx << q) | (1 << free) | rng.getrandbits(free) if free else (idx << q) | 1


TRIES = 64     # per k-mer: every search here is bounded (a canonical k = 32 target with rho >= q has no free bit at all)


def craft(k, p, idx, rho, rng, canonical):
    """A k-mer string (k >= 32) whose update is (idx, rho) at log2m p, or None.  canonical: the k-mer must also be the
    canonical one of its pair.  k = 32: the key is the k-mer, the only freedom is the tail behind the leading one;
    k >= 33: any high part works, the low word follows from it."""
    assert 32 <= k <= 64
    free_tail = rho < 64 - p
    for _ in range(TRIES):
        key = inv_wang64(target_hash(idx, rho, p, rng))
        if k == 32:
            s = kmer_str(key, 32)
        else:
            hi = rng.getrandbits(2 * k - 64)
            s = kmer_str((hi << 64) | (key ^ ((hi * G) & M64)), k)
        if not canonical or is_canonical(s):
            return s
        if k == 32 and not free_tail:
            return None
    return None


def crafted(k, p, canonical, seed, n_extra=0):
    """[(kmer, idx, rho)] for k >= 32: one k-mer per target of rho_targets(p), every one with a register index of its own;
    the q + 1 target is tried at index 0 first (the key whose hash is exactly 0).  A target that cannot be had at an index
    (k = 32 canonical) moves on to the next index; at most 4 * TRIES indices are tried per k-mer, and one that is still
    missing raises.  n_extra more k-mers follow with rho cycling through the targets >= 33, at indices of their own while
    there are any (log2m 4 has 16 registers); after that they share registers that already hold at least their rho, so
    that sharing never changes what a register ends as."""
    rng = random.Random((seed << 16) ^ (k << 8) ^ (p << 1) ^ int(canonical))
    m = 1 << p
    order = rng.sample(range(1, m), min(m - 1, 4096))
    best, out = {}, []

    def one(rho, candidates):
        for idx in candidates[:4 * TRIES]:
            s = craft(k, p, idx, rho, rng, canonical)
            if s is not None:
                best[idx] = max(rho, best.get(idx, 0))
                out.append((s, idx, rho))
                return
        raise AssertionError(f"no k-mer for k={k} log2m={p} rho={rho} canonical={canonical}")

    for rho in rho_targets(p):
        one(rho, [i for i in ([0] if rho == 64 - p + 1 else []) + order if i not in best])
    high = [r for r in rho_targets(p) if r >= 33]
    for i in range(n_extra):
        rho = high[i % len(high)]
        one(rho, [j for j in order if j not in best] or [j for j in [0] + order if best.get(j, 0) >= rho])
    return out


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_entries(k, p, canonical):
    """[(kmer, idx, rho)] of the searched k <= 31 k-mers usable in that strand mode"""
    return [(s, idx, rho) for kk, pp, s, canon_ok, idx, rho in load_fixture()["entries"]
            if kk == k and pp == p and (canon_ok or not canonical)]


# ---- the GPU tests' input --------------------------------------------------------------------------------------------------
FLANK = 9000    # bases on each side of the k-mers inside the long record: more than a wave's 64 x 64 tokens and its halo, so
                # every wave that holds one of them has no BREAK at all (the kernels' clean path)


def _bases(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def wave_records(kmers, rnd):
    """64 k-mers, each completed at the same token of 64 consecutive 64-token thread segments, so that the lanes of a wave
    reach them in the same step: k <= 63 as 64 records of 63 bases that end with the k-mer (+ the record's BREAK); k = 64 as
    one record of the 64 k-mers back to back."""
    assert len(kmers) == 64
    k = len(kmers[0])
    if k == 64:
        return ">wave\n" + "".join(kmers) + "\n"
    return "".join(f">wave{j}\n{_bases(rnd, 63 - k)}{s}\n" for j, s in enumerate(kmers))


def build_input(background, isolated, alone, waves, only_revcomp, rnd):
    """FASTA bytes: a background of >= 3 records (bytes) with, between and behind them,
       - `isolated` as a record of its own between the first two background records (no other made k-mer near: one lane),
       - every k-mer of `alone` as a record of exactly its k bases (next to a BREAK: the kernels' checked path), and the
         reverse complement of every k-mer of `only_revcomp`,
       - the wave sets (wave_records),
       - every k-mer of `alone` again inside ONE long record, FLANK random bases in front and behind and 97 between them."""
    recs = [b">" + r for r in bytes(background).split(b">")[1:]]
    assert len(recs) >= 3
    short = "".join(f">alone{j}\n{s}\n" for j, s in enumerate(alone))
    short += "".join(f">rc{j}\n{revcomp(s)}\n" for j, s in enumerate(only_revcomp))
    inside = ">inside\n" + _bases(rnd, FLANK) + "".join(s + _bases(rnd, 97) for s in alone) + _bases(rnd, FLANK) + "\n"
    parts = [recs[0], f">isolated\n{isolated}\n".encode(), recs[1], short.encode()]
    parts += [wave_records(w, rnd).encode() for w in waves]
    parts += recs[2:] + [inside.encode()]
    return b"".join(parts)
