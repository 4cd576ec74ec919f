"""GPU: sweep_kernel's per-wave raise queues (dd_k1.h: RaiseQueue), whole register slabs against the oracle byte for
byte.  log2m <= 16; the 64-, 96- and 128-bit window classes queue a rising register's record per wave and apply 64 at a
time, the 32-bit class and a group that fills its 80 KiB apply it at once.

  cold        one 70 000-base genome = two tiles, the second partial: nearly every lane of every step is a candidate, so the
              queue is bypassed; k 15..18 spans the 32-/64-bit classes, 31..34 the 64-/96-bit ones, 47..50 the 96-/128-bit ones
  four copies the same bases four times in one record, five tiles.  An input this small gets one tile per job and all its jobs
              start at once from the empty slab, so each is a cold job of its own (the copies only make them find the same
              registers); what they add to the cold case is more jobs whose dense start thins out into steps of a few
              candidates, i.e. appends, flushes of 64 and a part-filled queue at the drain, in every wave.  (A job that finds
              the slab warm needs a call of thousands of tiles: tests/test_gpu_fullsize.py and the benchmark run those.)
  breaks      nine records with N runs of 1, k - 1, k and 70 bases (the walk's CHECK variant), and 26 genomes of 5 kbp in one
              call (every job one partial tile, most lanes -- and most waves -- beyond the stream)
  rare rho    k-mers made with tests/rare_rho.py whose records carry rho - 1 = 32 - p - 1, 32 - p, 31 and, in the long form
              (the 32 bits behind the index all zero), rho >= 33: alone, inside a clean record and 64 at the same step of one wave
  no room     five ks of the 64-bit class at log2m 14 fill the 80 KiB: the plan gives no queue (tests/test_plan_raise_queue.py)"""
import functools
import random

import numpy as np
import pytest

import rare_rho
from test_gpu_parity import _sweep_check

pytestmark = pytest.mark.gpu

SEED = 0xD4ADD
K_RANGES = [(15, 18), (31, 34), (47, 50)]


def _bases(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def _one_record(n, copies):
    rnd = random.Random(f"sweep raises {n}")
    return np.frombuffer((">g\n" + _bases(rnd, n) * copies + "\n").encode(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _with_n_runs(k):
    rnd = random.Random(f"n runs {k}")
    recs = []
    for j, run in enumerate([1, k - 1, k, 70, 1, k - 1, k, 70, 2]):
        recs.append(f">r{j}\n{_bases(rnd, 3000 + 517 * j)}{'N' * run}{_bases(rnd, k - 1)}{'N' * run}{_bases(rnd, 4100 + 33 * j)}\n")
    return np.frombuffer("".join(recs).encode(), dtype=np.uint8)


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("p", [14, 16])
@pytest.mark.parametrize("krange", K_RANGES, ids=lambda r: f"k{r[0]}-{r[1]}")
def test_cold_job_bypasses_the_queue(engine_factory, orc, krange, p, canonical):
    _sweep_check(engine_factory(p, canonical), orc, _one_record(70_000, 1), *krange, canonical)


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("p", [14, 16])
@pytest.mark.parametrize("krange", K_RANGES, ids=lambda r: f"k{r[0]}-{r[1]}")
def test_four_copies_in_one_record(engine_factory, orc, krange, p, canonical):
    _sweep_check(engine_factory(p, canonical), orc, _one_record(70_000, 4), *krange, canonical)


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("p", [14, 16])
@pytest.mark.parametrize("krange", K_RANGES, ids=lambda r: f"k{r[0]}-{r[1]}")
def test_n_runs_take_the_checked_walk(engine_factory, orc, krange, p, canonical):
    _sweep_check(engine_factory(p, canonical), orc, _with_n_runs(krange[0] + 1), *krange, canonical)


@pytest.mark.parametrize("p", [14, 16])
def test_many_short_genomes_in_one_call(engine_factory, torch_cuda, orc, p):
    """26 x 5 kbp through dd_sketch_device: 79 live segments per genome, so wave 0 is whole, wave 1 part live, 14 are not"""
    torch = torch_cuda
    eng = engine_factory(p, True)
    fas = [orc.synth_fasta(SEED, 40 + g, 5_000, 1 + g % 3) for g in range(26)]
    for kmin, kmax in K_RANGES:
        K = kmax - kmin + 1
        bufs = []
        for fa in fas:
            t = torch.zeros(fa.size + 16, dtype=torch.uint8, device="cuda")
            t[:fa.size] = torch.from_numpy(fa)
            bufs.append(t)
        slab = torch.empty((len(fas), K, 1 << p), dtype=torch.uint8, device="cuda")
        eng.sketch_device([b.data_ptr() for b in bufs], [fa.size for fa in fas], kmin, kmax, slab.data_ptr())
        eng.synchronize()
        got = slab.cpu().numpy()
        for g, fa in enumerate(fas):
            assert np.array_equal(got[g], orc.sketch_sweep(fa, kmin, kmax, p, True)), (g, kmin, kmax)


def test_a_group_without_room_for_queues(engine_factory, orc):
    from dandd_amd.engine import plan_sweep
    fa = _one_record(70_000, 4)
    assert set(plan_sweep(14, [fa.size], 17, 21)["lds_bytes"]) == {80 * 1024}      # registers only
    assert set(plan_sweep(14, [fa.size], 17, 20)["lds_bytes"]) == {72 * 1024}      # (four ks: registers + queues)
    _sweep_check(engine_factory(14, True), orc, fa, 17, 21, True)
    _sweep_check(engine_factory(14, True), orc, _with_n_runs(18), 17, 21, True)


# ---- made k-mers: values round the hash words' boundary, and the long form ---------------------------------------------------------------
RARE_K = {"kc1": 32, "kc3": 40, "kc2": 56}


def rho_targets(p):
    """rho - 1 = 32 - p - 1 and 32 - p (the last bit of the high hash word, the first of the low one), 31 (the last value of
    the short form), then the long form: 33, 40 and an all-zero tail"""
    return [32 - p, 32 - p + 1, 32, 33, 40, 64 - p + 1]


@functools.lru_cache(maxsize=None)
def _rare_input(orc, cls, p, canonical):
    k = RARE_K[cls]
    rng = random.Random(f"sweep raises rare {cls} {p} {canonical}")
    free = rng.sample(range(1, 1 << p), 400)
    made = []

    def one(rho):
        while free:
            idx = free.pop()
            s = rare_rho.craft(k, p, idx, rho, rng, canonical)
            if s is not None:
                made.append((s, idx, rho))
                return True
        return False

    for rho in rho_targets(p):
        ok = one(rho)
        assert ok or (k == 32 and canonical and rho >= 64 - p), (k, p, rho)   # (a canonical 32-mer with no free tail bit may not exist)
    alone = list(made)
    wave = []
    while len(wave) < 64:
        n = len(made)
        assert one(rho_targets(p)[len(wave) % 5])
        wave.append(made[n][0])
    bg = orc.synth_fasta(SEED, 9, 200_000, 3)
    isolated = next(s for s, _, rho in alone if rho >= 33)
    fa = rare_rho.build_input(bg.tobytes(), isolated, [s for s, _, _ in alone], [wave], [], rng)
    return np.frombuffer(fa, dtype=np.uint8), k, made


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("p", [14, 16])
@pytest.mark.parametrize("cls", sorted(RARE_K))
def test_rare_rho_through_the_queue(engine_factory, orc, cls, p, canonical):
    fa, k, made = _rare_input(orc, cls, p, canonical)
    got = _sweep_check(engine_factory(p, canonical), orc, fa, k - 1, k + 1, canonical)
    want = orc.sketch_sweep(fa, k - 1, k + 1, p, canonical)
    rhos = set()
    for _, idx, rho in made:
        assert want[1, idx] == rho == got[1, idx], (idx, rho, want[1, idx], got[1, idx])
        rhos.add(rho)
    assert rhos >= set(rho_targets(p)[:5])
