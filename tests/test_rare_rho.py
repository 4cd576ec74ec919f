"""CPU: the oracle on k-mers whose update has rho >= 33 -- the searched ones of tests/golden/rare_rho.json (k <= 31) and
the ones tests/rare_rho.py makes to order (k >= 32) -- pinned with the independent pure-Python reference, before
tests/test_gpu_rare_rho.py asks the same of the kernels.  No GPU."""
import os
import random

import numpy as np
import pytest

import pyref
import rare_rho

FIXTURE_KS = [13, 14, 15, 16, 17, 20, 24, 28, 31]
CRAFT_KS = [32, 33, 40, 48, 49, 64]
LOG2M = [4, 10, 14, 16, 17, 18, 20]
SEED = 0xD4ADD


def _alone(s, k, p, canonical):
    return pyref.sketch(f">r\n{s}\n".encode(), k, p, canonical)


def _assert_exactly(regs, idx, rho):
    assert regs[idx] == rho and regs.count(0) == len(regs) - 1, (idx, rho, regs[idx])


def test_wang64_inverse():
    rnd = random.Random(5)
    for x in [0, 1, 2**64 - 1, 2**63] + [rnd.getrandbits(64) for _ in range(500)]:
        assert rare_rho.inv_wang64(pyref.wang64(x)) == x
        assert pyref.wang64(rare_rho.inv_wang64(x)) == x
    # three keys from the first scan that showed such k-mers exist (one each of k = 16, 20, 31)
    assert rare_rho.idx_rho_of(rare_rho.kmer_str(0xF3BB5482, 16), 20) == (353529, 34)
    assert rare_rho.idx_rho_of(rare_rho.kmer_str(0x405B04E55E, 20), 14) == (2010, 34)
    assert rare_rho.idx_rho_of(rare_rho.kmer_str(0x13EFBA35B004EA34, 31), 20) == (1048575, 33)


def test_fixture_is_what_the_generator_promises():
    fx = rare_rho.load_fixture()
    assert os.path.getsize(rare_rho.FIXTURE) < 100_000 and 100 <= len(fx["entries"]) <= 500
    per_pair = {}
    for k, p, s, canon_ok, idx, rho in fx["entries"]:
        assert k in FIXTURE_KS and len(s) == k and set(s) <= set("ACGT")
        assert canon_ok == rare_rho.is_canonical(s)
        assert rho >= 33 and 0 <= idx < (1 << p)
        per_pair.setdefault((k, p), []).append((idx, rho, s))
    for (k, p), v in per_pair.items():
        assert len({s for _, _, s in v}) == len(v)
        if k > 16:
            assert len(v) <= 8 and len({i for i, _, _ in v}) == len(v)      # distinct registers
            assert p in (10, 14, 16, 17, 18, 20) or (k, p) == (17, 4)
    # k <= 16 is exhaustive at every log2m 4..20: as many entries as the scan counted -- none at all for k <= 12, i.e. for
    # the k-mer-set classes (k <= 9 and k = 10, 11), and e.g. none for k = 16 at log2m 14
    for k in range(1, 17):
        for p in range(4, 21):
            assert len(per_pair.get((k, p), [])) == fx["counts"][str(k)][str(p)]
    assert fx["counts"]["16"]["14"] == 0 and fx["counts"]["16"]["20"] == 3
    s = rare_rho.kmer_str(0xF3BB5482, 16)
    assert [16, 20, s, rare_rho.is_canonical(s), 353529, 34] in fx["entries"]
    for k in range(1, 13):
        assert not any(fx["counts"][str(k)].values()), k
    # where a search had something to find, it kept some: every (k >= 20, log2m) pair is there with both rho 33 and a larger one
    for k in (20, 24, 28, 31):
        for p in (10, 14, 16, 17, 18, 20):
            rhos = {r for _, r, _ in per_pair[(k, p)]}
            assert 33 in rhos and max(rhos) > 33 and fx["counts"][str(k)][str(p)] >= len(per_pair[(k, p)])


@pytest.mark.parametrize("k", FIXTURE_KS)
def test_fixture_kmers_have_their_update(k):
    n = 0
    for kk, p, s, canon_ok, idx, rho in rare_rho.load_fixture()["entries"]:
        if kk != k:
            continue
        _assert_exactly(_alone(s, k, p, False), idx, rho)
        if canon_ok:
            _assert_exactly(_alone(s, k, p, True), idx, rho)
            _assert_exactly(_alone(rare_rho.revcomp(s), k, p, True), idx, rho)
        n += 1
    assert n > 0


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", CRAFT_KS)
def test_crafted_kmers_have_their_update(k, canonical):
    for p in LOG2M:
        made = rare_rho.crafted(k, p, canonical, SEED, n_extra=8)
        assert [r for _, _, r in made[:8]] == rare_rho.rho_targets(p)           # no target went missing
        assert len({i for _, i, _ in made[:8]}) == 8
        if not canonical:
            assert made[7][1] == 0 and pyref.wang64(rare_rho.key_of(made[7][0])) == 0   # the key whose hash is exactly 0
        for s, idx, rho in made:
            assert len(s) == k and (not canonical or rare_rho.is_canonical(s))
            _assert_exactly(_alone(s, k, p, canonical), idx, rho)


def test_crafting_gives_up_where_nothing_is_free():
    """k = 32 canonical with rho >= q: the hash fixes the k-mer, so one index either works or does not -- None, not a loop."""
    rng = random.Random(1)
    got = [rare_rho.craft(32, 14, idx, 50, rng, True) for idx in range(64)]
    assert any(g is None for g in got) and any(g is not None for g in got)
    for idx, g in enumerate(got):
        if g is not None:
            assert rare_rho.is_canonical(g) and rare_rho.idx_rho_of(g, 14) == (idx, 50)


def _records_fasta(kmers, canonical, rnd):
    """every k-mer as a record of its own and inside a longer record; in non-canonical mode their reverse complements too"""
    out = []
    for j, s in enumerate(kmers):
        out.append(f">alone{j}\n{s}\n")
        flank = ["".join(rnd.choice("ACGT") for _ in range(64 + j)) for _ in range(2)]
        out.append(f">inside{j}\n{flank[0]}{s}{flank[1]}\n")
        if not canonical:
            out.append(f">rc{j}\n{rare_rho.revcomp(s)}\n")
    return "".join(out).encode()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", FIXTURE_KS + CRAFT_KS)
def test_oracle_matches_python_on_rare_rho(orc, k, canonical):
    rnd = random.Random(k)
    pairs = 0
    for p in range(4, 21) if k <= 16 else LOG2M:
        made = rare_rho.crafted(k, p, canonical, SEED) if k >= 32 else rare_rho.fixture_entries(k, p, canonical)
        if not made:
            continue
        fa = _records_fasta([s for s, _, _ in made], canonical, rnd)
        want = pyref.sketch(fa, k, p, canonical)
        for s, idx, rho in made:
            assert want[idx] == rho, (k, p, s)
        buf = np.frombuffer(fa, dtype=np.uint8)
        assert list(orc.sketch(buf, k, p, canonical)) == want
        assert list(orc.sketch_generic(buf, k, p, canonical)) == want
        lo, hi = max(1, k - 1), min(64, k + 1)
        assert list(orc.sketch_sweep(buf, lo, hi, p, canonical)[k - lo]) == want      # (what the GPU tests compare with)
        pairs += 1
    assert pairs > 0
