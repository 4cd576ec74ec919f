"""GPU: register updates with rho >= 33 on every K1 family, bit-for-bit against the oracle.

rho(h) is ffbh + 1 of the 32 hash bits behind the register index; when those are all zero (one hash in 2^32: no parity
input is long enough to meet one) the kernels take a second form behind a wave-level branch (dd_k1.h: rho_of), and their
callers rely on conventions of their own around it -- the unsigned compare `lz >= bound` with lz = 0xFFFFFFFF, rho - 1 in
the low byte of a queue word with 0xFF for "no candidate", records as idx | rho << 24.  These inputs hold k-mers MADE to
have such hashes (tests/rare_rho.py; tests/test_rare_rho.py pins the oracle on them with the pure-Python reference):

  k <= 31   searched ones from tests/golden/rare_rho.json: every k-mer of k <= 16 that exists (k = 13 .. 16 only: there
            is none for k <= 12, so the k-mer-set classes -- bitmaps for k <= 9, exact sets for k = 10, 11 -- cannot be
            reached; their finishers use the same probe / rho_of / hll_update as the classes here), up to 8 per
            (k, log2m) for k = 17, 24, 31
  k >= 32   made to order, one per target rho: 31, 32 (the last values of the short form), 33, 34, 40, q - 1, q, q + 1 (an
            all-zero tail; 61 at log2m 4 is the largest value a register can hold), each at a register of its own, the
            q + 1 one at register 0 where the strand mode allows (the key whose hash is 0); 64 more with rho >= 33 for
            the wave set

each placed (rare_rho.build_input) as a record of exactly k bases, alone between two background records (one lane of a
wave), inside a long clean record (the wave-uniform path without BREAKs), and in a set of 64 records whose k-mers the
lanes of one wave complete in the same step (k <= 31: the few there are, repeated); in non-canonical mode one more k-mer
(k >= 32, log2m >= 10) is placed ONLY as its reverse complement and must not show.  The background (200 000 bases, three
records) gives the made updates warm registers, filters and queues to meet.

Every case sweeps k - 1 .. k + 1 round each k that has something placed, so that a made update is paired both ways in
hll_update2, and checks (1) all registers == the oracle's, (2) the oracle's -- and the engine's -- register at every made
k-mer's index is exactly the rho it was made for, (3) as many registers with rho >= 33 were checked as were placed.

Nothing to place (the searches found nothing; tests/golden/rare_rho.json "counts"), so not covered:
  k = 13, 14: every log2m but 16, 17, 18;  k = 15: every log2m but 12, 13, 16, 17, 18;  k = 16 at log2m 8, 9, 14 (count 0) --
  of the log2m values used here that is k = 16 at log2m 14 and k = 13 .. 15 at log2m 4, 10, 14, 20;
  in canonical mode, where a k-mer must also be the smaller of its pair: k = 13 .. 16 at log2m 4, 10, 20 and k = 17 at log2m 14;
  k = 24, 31 at log2m 4 (searched at log2m 10, 14, 16, 17, 18, 20 only; k = 17 and k >= 32 are there).
test_nothing_is_left_out_silently holds the same list as data."""
import functools
import random

import numpy as np
import pytest

import rare_rho
from test_gpu_parity import BUCKET_KNOBS, _sweep_check

pytestmark = pytest.mark.gpu

SEED = 0xD4ADD
CLASS_KS = {"kc0": [13, 14, 15, 16], "kc1": [17, 24, 31, 32], "kc3": [33, 40, 48], "kc2": [49, 64]}
BACKGROUND_GENOME = {"kc0": 4, "kc1": 5, "kc3": 6, "kc2": 7}
# log2m 4 .. 16: sweep_kernel, registers in LDS; 17: the record path; 18, 20: binned first epoch (records idx | rho << 24),
# every tile an epoch of its own (filter, candidate queue with rho - 1 in the low byte, scatter_probe), a stream of one chunk
# (compare-and-swap fallback)
P_KNOBS = [(4, "default"), (10, "default"), (14, "default"), (16, "default"), (17, "default")] + \
          [(p, kn) for p in (18, 20) for kn in ("default", "many_epochs", "overflow")]
# (k class, log2m, strand mode) with nothing to place: see the docstring
NOTHING_TO_PLACE = {("kc0", 14, False), ("kc0", 4, True), ("kc0", 10, True), ("kc0", 14, True), ("kc0", 20, True)}


def _made(k, p, canonical):
    """-> (k-mers placed alone and inside [(s, idx, rho)], 64 for the wave set or [], the one placed as reverse complement only or None)"""
    if k >= 32:
        made = rare_rho.crafted(k, p, canonical, SEED, n_extra=65)
        decoy = made[72] if not canonical and p >= 10 else None    # (log2m 4 has no register to spare for it)
        return made[:8], made[8:72], decoy
    fx = rare_rho.fixture_entries(k, p, canonical)
    return fx, [fx[i % len(fx)] for i in range(64)] if fx else [], None


@functools.lru_cache(maxsize=4)
def _case_input(orc, cls, p, canonical):
    """-> (FASTA bytes, {k: {idx: rho}} expected registers, {k: (idx, rho)} that must NOT show)"""
    rnd = random.Random(f"{cls} {p} {canonical}")
    alone, waves, decoys, expected, absent = [], [], [], {}, {}
    for k in CLASS_KS[cls]:
        prim, wave, decoy = _made(k, p, canonical)
        alone += [s for s, _, _ in prim]
        if wave:
            waves.append([s for s, _, _ in wave])
        for s, idx, rho in prim + wave:
            assert len(s) == k
            expected.setdefault(k, {})[idx] = max(rho, expected.get(k, {}).get(idx, 0))
        if decoy:
            assert decoy[1] not in expected[k]
            decoys.append(decoy[0])
            absent[k] = (decoy[1], decoy[2])
    if not alone:
        return None, expected, absent
    isolated = next(s for k in CLASS_KS[cls] for s, _, rho in _made(k, p, canonical)[0] if rho >= 33)
    bg = orc.synth_fasta(SEED, BACKGROUND_GENOME[cls], 200_000, 3)
    fa = rare_rho.build_input(bg.tobytes(), isolated, alone, waves, decoys, rnd)
    return np.frombuffer(fa, dtype=np.uint8), expected, absent


def _has_input(cls, p, canonical):
    return any(_made(k, p, canonical)[0] for k in CLASS_KS[cls])


def _cases():
    out = []
    for cls in ("kc1", "kc3", "kc2"):
        out += [(cls, p, kn, canonical) for p, kn in P_KNOBS for canonical in (True, False)]
    # k <= 16: where the fixture has something; the knob variants in non-canonical mode, where there is the most
    for p, kn in P_KNOBS + [(18, "exact_sets"), (20, "exact_sets")]:
        out += [("kc0", p, kn, canonical) for canonical in (False, True)
                if _has_input("kc0", p, canonical) and (kn == "default" or not canonical)]
    return out


CASES = _cases()


def test_nothing_is_left_out_silently():
    """The cases are every (class, log2m, knobs, strand mode) but those of NOTHING_TO_PLACE, and in the others every k of the
    class has k-mers but the (k, log2m, strand mode) the docstring names."""
    assert 60 <= len(CASES) <= 85
    all_p = sorted({p for p, _ in P_KNOBS})
    missing = {(cls, p, canonical) for cls in CLASS_KS for p in all_p for canonical in (True, False) if not _has_input(cls, p, canonical)}
    assert missing == NOTHING_TO_PLACE
    assert {(c, p, cn) for c, p, _, cn in CASES} == {(cls, p, cn) for cls in CLASS_KS for p in all_p for cn in (True, False)} - missing
    empty = {(k, p, cn) for cls in CLASS_KS for k in CLASS_KS[cls] for p in all_p for cn in (True, False)
             if (cls, p, cn) not in missing and not _made(k, p, cn)[0]}
    assert empty == ({(k, p, cn) for k in (13, 14, 15) for p in (4, 10, 20) for cn in (False,)}
                     | {(24, 4, cn) for cn in (True, False)} | {(31, 4, cn) for cn in (True, False)} | {(17, 14, True)})


@pytest.mark.parametrize("cls,p,knobs,canonical", CASES, ids=[f"{c}-p{p}-{kn}-{'canon' if cn else 'fwd'}" for c, p, kn, cn in CASES])
def test_rare_rho_registers(engine_factory, orc, monkeypatch, cls, p, knobs, canonical):
    for name, v in BUCKET_KNOBS[knobs].items():
        monkeypatch.setenv(name, v)
    fa, expected, absent = _case_input(orc, cls, p, canonical)
    assert fa is not None and 200_000 < fa.size < 320_000
    eng = engine_factory(p, canonical)
    placed_high = {(k, idx) for k, regs in expected.items() for idx, rho in regs.items() if rho >= 33}
    assert placed_high, "a case without a single rho >= 33 k-mer"
    if cls != "kc0":
        assert {rho for regs in expected.values() for rho in regs.values()} >= set(rare_rho.rho_targets(p))
    if knobs == "exact_sets":
        # DD_BIGMAP_ANY_SIZE makes k = 10 (, 11) exact k-mer sets; the planner has NO set class for k >= 12, whatever the knobs,
        # so the k = 13 .. 16 k-mers of this case go through the hashed class here as well (asserted; the case stays as the
        # record that it was looked at)
        from dandd_amd.engine import plan_sweep
        assert (plan_sweep(p, [fa.size], 12, 17)["kclass"] >= 0).all()
        assert (plan_sweep(p, [fa.size], 10, 10)["kclass"] < 0).all() == (p >= 19)
    checked = set()
    ranges = sorted({(max(1, k - 1), min(64, k + 1)) for k in expected})
    for lo, hi in ranges:
        got = _sweep_check(eng, orc, fa, lo, hi, canonical)
        want = orc.sketch_sweep(fa, lo, hi, p, canonical)
        for k in range(lo, hi + 1):
            for idx, rho in expected.get(k, {}).items():
                assert want[k - lo, idx] == rho, f"the oracle's register (k={k}, idx={idx}) is {want[k - lo, idx]}, the k-mer placed there has rho {rho}"
                assert got[k - lo, idx] == rho
                if rho >= 33:
                    checked.add((k, idx))
            if k in absent:
                idx, rho = absent[k]
                assert want[k - lo, idx] < 31 and got[k - lo, idx] == want[k - lo, idx], (k, idx, rho)
    assert checked == placed_high and len(checked) >= len(placed_high)
