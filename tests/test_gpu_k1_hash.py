"""GPU: the Wang mix as the K1 kernels arrange it (the multiply by 265 folded into one mad) and their register probe (dd_k1.h: mul64_c32_fold, probe, RegsLds::at),
whole register slabs against the oracle byte for byte, on k-mers MADE to sit where that arithmetic can go wrong.  Every made
k-mer is a FASTA record of exactly its k bases, so it is the one k-mer of that k the record holds (smaller ks of the range
see its sub-k-mers, which the oracle sees as well).

  k = 32 (64-bit class)  keys whose value ENTERING the multiply by 265 is every pair of the edge words 0, 1, 0x7FFFFFFF,
             0x80000000, 0xFFFFFFFF, 0x00F0F0F1 (the first two steps of the mix run backwards, as rare_rho.inv_wang64 does): the
             largest carry out of lo * 265 and hi * 265 with hi = 0xFFFFFFFF among them.  In canonical mode a record is hashed
             as the smaller of the key and its reverse complement: the keys that are canonical themselves are counted.
  k = 16 (32-bit class: the first multiply takes its HI_ZERO form)  keys from a seeded search over 2^18 + 2^11 candidates
             whose value entering the multiply by 265 has lo * 265 carrying >= 263, and the keys below 2^11 whose value there has
             a zero high word.
  k = 33 .. 40 (96-bit class) and k = 32  rare_rho.craft: a k-mer for register 0 and one for register m - 1 of EVERY k of the
             group, with a short-form rho and with rho = 33 (hiw == 0) -- the first and the last register of every slot, the
             last slot's being the highest register address below the raise queues.

  log2m 14   k ranges that make groups of 1, 2, 3 and 4 ks (asserted on the plan); log2m 12: many slots per group; log2m 16: one
             slot; log2m 4; and log2m 17 on the k = 32 keys: the scatter kernels share the hash.

Every case asserts how many made k-mers it placed and that the oracle's register at each one's index holds at least its rho."""
import functools
import random

import numpy as np
import pytest

import pyref
import rare_rho
from test_gpu_parity import _sweep_check

pytestmark = pytest.mark.gpu

M64 = pyref.M64
EDGE = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x00F0F0F1]
SEED = 0x17C0DE


def _key_before_265(y):
    """the key whose value entering the multiply by 265 is y"""
    return ((rare_rho._unxorshift(y, 24) + 1) * rare_rho._INV_2P21M1) & M64


def _enters_265(x):
    z = ((~x & M64) + (x << 21)) & M64
    return z ^ (z >> 24)


@functools.lru_cache(maxsize=None)
def _edge_keys32():
    """36 32-mers, one per pair of edge words"""
    out = []
    for hi in EDGE:
        for lo in EDGE:
            x = _key_before_265((hi << 32) | lo)
            assert _enters_265(x) == (hi << 32) | lo
            out.append(rare_rho.kmer_str(x, 32))
    assert len(set(out)) == 36
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _carry_keys16():
    """(16-mers whose lo * 265 carries >= 263 into the high word, 16-mers whose value entering that multiply has hi == 0)"""
    rnd = np.random.RandomState(SEED)
    x = np.concatenate([np.arange(1 << 11, dtype=np.uint64), rnd.randint(0, 1 << 32, size=1 << 18, dtype=np.uint64)])
    z = x * np.uint64((1 << 21) - 1) - np.uint64(1)                 # (x < 2^32: no wrap, but uint64 arithmetic wraps as the mix does)
    y = z ^ (z >> np.uint64(24))
    carry = ((y & np.uint64(0xFFFFFFFF)) * np.uint64(265)) >> np.uint64(32)
    hi0 = (y >> np.uint64(32)) == 0
    carries = [int(v) for v in x[carry >= 263][:64]]
    zero_hi = [int(v) for v in x[hi0][-24:]] + [int(v) for v in x[hi0 & (carry >= 263)]]
    for v in carries:
        assert ((_enters_265(v) & 0xFFFFFFFF) * 265) >> 32 >= 263
    for v in zero_hi:
        assert _enters_265(v) >> 32 == 0
    assert len(carries) == 64 and len(zero_hi) >= 24 and any(((_enters_265(v) & 0xFFFFFFFF) * 265) >> 32 >= 263 for v in zero_hi)
    return tuple(rare_rho.kmer_str(v, 16) for v in carries), tuple(rare_rho.kmer_str(v, 16) for v in dict.fromkeys(zero_hi))


@functools.lru_cache(maxsize=None)
def _crafted(k, p, canonical):
    """[(kmer, idx, rho)]: register 0 and register m - 1, each with a short-form rho and with rho = 33"""
    rng = random.Random(f"k1 hash {k} {p} {canonical}")
    out = []
    for idx in (0, (1 << p) - 1):
        for rho in (3, 33):
            s = rare_rho.craft(k, p, idx, rho, rng, canonical)
            assert s is not None and len(s) == k and rare_rho.idx_rho_of(s, p) == (idx, rho)
            out.append((s, idx, rho))
    return tuple(out)


def _fasta(kmers):
    return np.frombuffer("".join(f">r{j}\n{s}\n" for j, s in enumerate(kmers)).encode(), dtype=np.uint8)


def _check(eng, orc, kmers, kmin, kmax, canonical, expect_placed):
    """kmers: the made k-mers; -> (registers, how many of them are hashed as themselves: each of those must show in the registers)"""
    p = eng.log2m
    assert len(kmers) == expect_placed, f"{len(kmers)} made k-mers, the case is written for {expect_placed}"
    fa = _fasta(kmers)
    got = _sweep_check(eng, orc, fa, kmin, kmax, canonical)
    seen = 0
    for s in kmers:
        k = len(s)
        assert kmin <= k <= kmax
        if canonical and not rare_rho.is_canonical(s):
            continue
        idx, rho = rare_rho.idx_rho_of(s, p)
        assert got[k - kmin, idx] >= rho, (s, idx, rho)
        seen += 1
    return got, seen


def _group_sizes(p, nbytes, kmin, kmax, kclass):
    from dandd_amd.engine import plan_sweep
    jobs = plan_sweep(p, [nbytes], kmin, kmax)
    return sorted({int(j["nk"]) for j in jobs if j["kclass"] == kclass})


N_CANON32 = sum(rare_rho.is_canonical(s) for s in _edge_keys32())


@pytest.mark.parametrize("canonical", [False, True], ids=["fwd", "canon"])
@pytest.mark.parametrize("p,kmin", [(14, 32), (14, 31), (14, 30), (14, 29), (12, 17), (16, 32), (4, 29), (17, 31)],
                         ids=lambda v: str(v))
def test_k32_edge_pairs_into_the_multiply_by_265(engine_factory, orc, p, kmin, canonical):
    """64-bit class: groups of 1 .. 4 ks at log2m 14 with k = 32 in the LAST slot (its register m - 1 is the highest address
    below the raise queues), 16 slots at log2m 12, one at log2m 16, log2m 4, and the record path at log2m 17"""
    eng = engine_factory(p, canonical)
    kmers = list(_edge_keys32()) + [s for s, _, _ in _crafted(32, p, canonical)]
    if p == 14:
        assert _group_sizes(p, _fasta(kmers).size, kmin, 32, 1) == [32 - kmin + 1]
    if p == 12:
        assert _group_sizes(p, _fasta(kmers).size, kmin, 32, 1) == [16]
    if p == 16:
        assert _group_sizes(p, _fasta(kmers).size, kmin, 32, 1) == [1]
    _, seen = _check(eng, orc, kmers, kmin, 32, canonical, 36 + 4)
    assert 12 <= N_CANON32 <= 24                       # (about half of 36 random-looking 32-mers)
    assert seen == (N_CANON32 if canonical else 36) + 4


@pytest.mark.parametrize("canonical", [False, True], ids=["fwd", "canon"])
@pytest.mark.parametrize("p,kmin", [(14, 16), (14, 15), (14, 14), (12, 10), (16, 16), (4, 14)], ids=lambda v: str(v))
def test_k16_carries_out_of_the_low_product(engine_factory, orc, p, kmin, canonical):
    """32-bit class (HI_ZERO first multiply, the folded multiply by 265 behind it): groups of 1, 2, 3 ks at log2m 14"""
    eng = engine_factory(p, canonical)
    carries, zero_hi = _carry_keys16()
    kmers = list(carries) + list(zero_hi)
    if p == 14:
        assert _group_sizes(p, _fasta(kmers).size, kmin, 16, 0) == [16 - kmin + 1]
    _, seen = _check(eng, orc, kmers, kmin, 16, canonical, 64 + len(zero_hi))
    n_canon = sum(rare_rho.is_canonical(s) for s in kmers)
    assert n_canon >= 16 and seen == (n_canon if canonical else len(kmers))


@pytest.mark.parametrize("canonical", [False, True], ids=["fwd", "canon"])
@pytest.mark.parametrize("p,kmin,kmax", [(14, 33, 33), (14, 33, 34), (14, 33, 35), (14, 33, 36), (14, 40, 40), (12, 33, 40),
                                         (16, 33, 33), (16, 40, 40), (4, 33, 40)], ids=lambda v: str(v))
def test_k33_40_first_and_last_register_of_every_slot(engine_factory, orc, p, kmin, kmax, canonical):
    """96-bit class: every k of the range (every slot of its group) has a k-mer at register 0 and one at register m - 1, with a
    short-form rho and with rho = 33; at log2m 14 groups of 1, 2, 3 and 4 ks"""
    eng = engine_factory(p, canonical)
    made = [t for k in range(kmin, kmax + 1) for t in _crafted(k, p, canonical)]
    kmers = [s for s, _, _ in made]
    if p == 14:
        assert _group_sizes(p, _fasta(kmers).size, kmin, kmax, 3) == [kmax - kmin + 1]
    if p == 12:
        assert _group_sizes(p, _fasta(kmers).size, kmin, kmax, 3) == [8]
    got, seen = _check(eng, orc, kmers, kmin, kmax, canonical, 4 * (kmax - kmin + 1))
    assert seen == len(kmers)
    for s, idx, rho in made:
        assert got[len(s) - kmin, idx] >= rho
        if rho == 33:
            assert got[len(s) - kmin, idx] == 33      # (nothing else in the input reaches 33)
