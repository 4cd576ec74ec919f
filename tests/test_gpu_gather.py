"""dd_exact_gather on the MI355X: every cell of pick / unique / depth / shared / total compared with == against gather_ref (the
loop of include/dandd_hip.h over depth_ref's counts) over test_gpu_screen's universe and samples in both strand modes; a
universe of 64 inputs with mixtures for samples (bit 63, lane 63, a close relative of a pick); ties and duplicates; both
stop rules; the identities with dd_exact_screen and dd_exact_depth; samples taken in rounds; records accumulated over
passes; two calls byte for byte; the device form; the argument rules; degenerate inputs; and `screen --gather` end to end
on a real `--exact` tree."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gather_ref
import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_gpu_screen as gs
import test_screen as cpus
from test_gather import read_gather

pytestmark = pytest.mark.gpu

N = gs.N
DD_EINVAL = -1


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("gather_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_samples")
    paths = []
    for name, raw, _ in gs.samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


def arrays(got):
    """what gather_ref gives for a list of samples -> the entry's five arrays"""
    return (np.array([g[0] for g in got], dtype=np.int32), *(np.array([g[j] for g in got], dtype=np.uint64) for j in (1, 2, 3, 4)))


def same(got, want, why=None):
    for name, g, w in zip(("pick", "unique", "depth", "shared", "total"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tolist() == w.tolist(), (name, why)


@functools.lru_cache(maxsize=None)
def want(k, canonical, min_hits=1, steps=N):
    """-> (the five arrays of S0..S6, found) from gather_ref: a computation of its own, never changed"""
    masks = cpur.reference(k, canonical)[1]
    return arrays([gather_ref.answer(text, k, canonical, masks, N, min_hits, steps) for _, _, text in gs.samples()]), len(masks)


# ---- 1. every cell against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in gs.KS] + [(False, k) for k in gs.KS_NOCANON])
def test_every_cell_equals_the_reference(engine_factory, fixture_paths, sample_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    got = eng.exact_gather(fixture_paths, sample_paths, k, min_hits=1, steps=N)
    assert eng.last_sketch_stats()[2] == 1
    w, w_found = want(k, canonical)
    assert eng.last_gather_found == w_found
    assert [a.shape for a in got] == [(7, N), (7, N), (7, N), (7, N), (7, 2)]
    same(got, w, (k, canonical))
    pick, unique, depth, shared, total = got
    # the fixture does what it is for: S0 is g0 byte for byte, and g4 is g0 again -- picked first, g4 never; S3 holds nothing
    assert pick[0, 0] == 0 and 4 not in pick[0].tolist() and shared[0, 0] == shared[0, 4] == unique[0, 0]
    assert (pick[3] == -1).all() and not total[3].any() and total[2, 1] > 4 * total[2, 0] > 0     # S2: reads that overlap, deep
    assert (pick[1] >= 0).sum() >= 2                                       # S1, a relative of the ancestor, takes more than one genome


# ---- 2. a universe of 64 inputs ----------------------------------------------------------------------------------------------
BIG_KS = (21, 33)


def _text(codes):
    return "".join("ACGT"[c] for c in codes)


@functools.lru_cache(maxsize=None)
def big():
    """-> (64 FASTA buffers of about 2 kbp -- a shared ancestor of 1000 bases mutated at 3 per cent, then a private stretch of
    1000 (g3: 1300, g63: 1150); g4 is g3 with one base in a hundred changed --, [(name, FASTA bytes of a mixture)])"""
    rng = np.random.default_rng(6463)
    anc = rng.integers(0, 4, 1000)
    seqs = []
    for i in range(64):
        s = anc.copy()
        mut = rng.random(len(s)) < 0.03
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        seqs.append((_text(s), _text(rng.integers(0, 4, {3: 1300, 63: 1150}.get(i, 1000)))))
    g3 = np.array(["ACGT".index(c) for c in seqs[3][0] + seqs[3][1]])
    mut = rng.random(len(g3)) < 0.01
    g3[mut] = (g3[mut] + 1 + rng.integers(0, 3, int(mut.sum()))) % 4
    seqs[4] = (_text(g3[:1000]), _text(g3[1000:]))
    fas = [gs.fasta(a + b, f"g{i}", 80) for i, (a, b) in enumerate(seqs)]
    whole = lambda i: seqs[i][0] + seqs[i][1]
    records = lambda name, texts: "".join(f">{name}{j}\n{t}\n" for j, t in enumerate(texts)).encode()
    mix1 = records("a", [whole(3), whole(40), whole(63), whole(40), seqs[10][1]])      # g40's text twice, g10's private half
    mix2 = records("b", [whole(3), whole(20), whole(50)[700:1300]])                     # g4, g3's relative, is in the universe
    return fas, [("mix1.fa", mix1), ("mix2.fa", mix2)]


@functools.lru_cache(maxsize=None)
def big_masks(k):
    return cpuc.masks_of(big()[0], k)


@functools.lru_cache(maxsize=None)
def big_want(k, min_hits=1, steps=64):
    return arrays([gather_ref.answer(text, k, True, big_masks(k), 64, min_hits, steps) for _, text in big()[1]])


@pytest.fixture(scope="module")
def big_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_big")
    fas, samples = big()
    return greedy.write(d, fas), greedy.write(d, [raw for _, raw in samples], tag="mix")


@pytest.mark.parametrize("k", BIG_KS)
def test_sixty_four_inputs(engine_factory, big_paths, k):
    eng = engine_factory()
    paths, smp = big_paths
    got = eng.exact_gather(paths, smp, k)                                   # (min_hits 1, steps None: all 64)
    w = big_want(k)
    assert eng.last_gather_found == len(big_masks(k)) > 80_000              # 1300 groups of 64 records and more, 16 to a wave: the loop strides
    same(got, w, k)
    # the fixture does what it is for, from the reference alone
    pick, unique, depth, shared, total = (a.tolist() for a in w)
    assert pick[0][:3] == [3, 63, 40] and 10 in pick[0][3:5]               # by size; g10's half behind them
    t40 = pick[0].index(40)
    assert depth[0][t40] == 2 * unique[0][t40] > 1500                       # g40 twice over: a mean depth of 2
    assert shared[0][63] > 1000 and unique[0][1] < shared[0][63]            # bit 63 counts, and loses what g3 took
    order = sorted(range(64), key=lambda b: -shared[1][b])
    assert order[:4] == [3, 20, 4, 50] and shared[1][4] > 2 * shared[1][50]   # the relative ranks above a genome of the mixture in shared
    assert pick[1][:4] == [3, 20, 50, -1]                                   # ... and is no pick: it adds nothing behind g3
    for s in range(2):
        assert sum(unique[s]) == total[s][0] and sum(depth[s]) == total[s][1]
        assert -1 in pick[s] and len(set(p for p in pick[s] if p >= 0)) == pick[s].index(-1) >= 3


# ---- 3. ties and duplicates ----------------------------------------------------------------------------------------------------
def test_duplicates_and_ties(engine_factory, tmp_path):
    eng = engine_factory()
    k = 21
    fam = greedy.related(6, 3000, 25)
    twin = greedy.related(1, 3300, 26)[0]                                   # longer than the others: the first pick
    fas = [fam[0], fam[1], twin, fam[3], fam[4], twin]                      # byte-identical at 2 and 5
    paths = greedy.write(tmp_path, fas)
    sample = twin + fam[1]
    (tmp_path / "s.fa").write_bytes(sample)
    masks = cpuc.masks_of(fas, k)
    w = arrays([gather_ref.answer(sample, k, True, masks, 6)])
    assert w[0][0, 0] == 2 and 5 not in w[0][0].tolist() and w[3][0, 2] == w[3][0, 5] and w[0][0, 1] == 1
    same(eng.exact_gather(paths, [str(tmp_path / "s.fa")], k), w)
    # two disjoint random inputs of the same length: U_0 ties, the lower index goes first
    rng = np.random.default_rng(27)
    a, b = (gs.fasta(_text(rng.integers(0, 4, 1500)), name) for name in "ab")
    pair = greedy.write(tmp_path, [a, b], tag="t")
    (tmp_path / "ab.fa").write_bytes(b + a)
    masks = cpuc.masks_of([a, b], k)
    w = arrays([gather_ref.answer(b + a, k, True, masks, 2)])
    assert w[3][0].tolist() == [1480, 1480] and w[0][0].tolist() == [0, 1] and w[1][0].tolist() == [1480, 1480]
    same(eng.exact_gather(pair, [str(tmp_path / "ab.fa")], k), w)


# ---- 4. the stop rules -----------------------------------------------------------------------------------------------------------
def test_stop_rules(engine_factory, big_paths):
    eng = engine_factory()
    paths, smp = big_paths
    k = 21
    full = big_want(k)
    for steps in (1, 2):
        got = eng.exact_gather(paths, smp, k, steps=steps)
        same(got, big_want(k, 1, steps), steps)
        assert got[0].shape == (2, steps) and got[0].tolist() == full[0][:, :steps].tolist() and got[3].tolist() == full[3].tolist()
    # min_hits between the second and the third pick's unique of mix1, as the reference has them
    second, third = int(full[1][0, 1]), int(full[1][0, 2])
    assert second > third + 1
    min_hits = third + 1
    got = eng.exact_gather(paths, smp, k, min_hits=min_hits)
    same(got, big_want(k, min_hits, 64), min_hits)
    pick, unique, depth = got[:3]
    assert pick[0, :2].tolist() == full[0][0, :2].tolist() and (pick[0, 2:] == -1).all() and not unique[0, 2:].any() and not depth[0, 2:].any()
    assert depth[0, 1] == full[2][0, 1] > 0                                 # the last pick's depth is closed behind the stop
    got = eng.exact_gather(paths, smp, k, min_hits=1 << 31)
    assert (got[0] == -1).all() and not got[1].any() and not got[2].any() and got[3].tolist() == full[3].tolist() and got[4].tolist() == full[4].tolist()


# ---- 5. identities with entry points that exist ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_identities_with_screen_and_depth(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    ns = len(sample_paths)
    pick, unique, depth, shared, total = eng.exact_gather(fixture_paths, sample_paths, k)
    sc_shared, sc_match = eng.exact_screen(fixture_paths, sample_paths, k, [0], [0])
    assert eng.last_gather_found == eng.last_screen_found
    assert shared.tolist() == sc_shared[:ns].tolist()
    assert total[:, 0].tolist() == sc_match[:ns, 0].tolist()
    _, d_total = eng.exact_depth(fixture_paths, sample_paths, k, [0], [0], bins=8)
    assert total[:, 1].tolist() == d_total[:, N].tolist()
    assert unique.sum(1).tolist() == total[:, 0].tolist() and depth.sum(1).tolist() == total[:, 1].tolist()
    assert (unique[:, 1:] <= unique[:, :-1]).all() and total[2, 1] > 30_000 and total[0, 0] > 5000
    assert ((pick >= 0) == (unique > 0)).all()


# ---- 6. samples taken in rounds, records accumulated over passes -----------------------------------------------------------
@pytest.mark.parametrize("k", [33, 61])
def test_seventy_samples_in_rounds(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    many = [sample_paths[j % 7] for j in range(70)]
    assert "DD_DEPTH_MB" not in os.environ
    os.environ["DD_DEPTH_MB"] = "1"
    try:
        got = eng.exact_gather(fixture_paths, many, k)
    finally:
        del os.environ["DD_DEPTH_MB"]
    found = eng.last_gather_found
    per = (1 << 20) // (found * 4)                                          # a sample's counters, and a few hundred bytes of its walk
    assert 1 <= per <= 17 and -(-70 // per) >= 5, (found, per)
    assert [a.shape for a in got] == [(70, N), (70, N), (70, N), (70, N), (70, 2)]
    for j in range(7):
        one = eng.exact_gather(fixture_paths, [sample_paths[j]], k)
        assert eng.last_gather_found == found
        for row in range(j, 70, 7):
            assert all(a[row].tobytes() == b[0].tobytes() for a, b in zip(got, one)), (k, row)
    w, _ = want(k, True)
    same([a[:7] for a in got], w)
    same([a[63:] for a in got], w)


@pytest.mark.parametrize("k", [13, 62])
def test_multi_pass_gives_identical_bytes(engine_factory, tmp_path, k):
    """test_gpu_screen's 17 x 19 kbp universe with a 1 MiB sort budget: at least three passes append their records before the
    one ordering the samples are walked against."""
    eng = engine_factory()
    family = greedy.related(18, 19_000, 17)
    paths = greedy.write(tmp_path, family[:17])
    other = greedy.write(tmp_path, family[17:], tag="x")
    smp = [paths[5], other[0]]
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_gather(paths, smp, k)
    found = eng.last_gather_found
    assert eng.last_sketch_stats()[2] == 1
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = eng.exact_gather(paths, smp, k)
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_gather_found > 65_536
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, many))
    pick, unique, depth, shared, total = one
    assert pick[0, 0] == 5 and (pick[0, 1:] == -1).all() and unique[0, 0] == total[0, 0] == shared[0, 5]   # a genome of the universe: one pick
    assert (pick[1] >= 0).sum() >= 2 and unique[1].sum() == total[1, 0]


# ---- 7. two calls, the device form -------------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(engine_factory, fixture_paths, sample_paths):
    eng = engine_factory()
    a = eng.exact_gather(fixture_paths, sample_paths, 29)
    b = eng.exact_gather(fixture_paths, sample_paths, 29)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].any()
    same(a, want(29, True)[0])


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = gs.samples()[2][2]
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    for k in (21, 62):
        dev = eng.exact_gather_device(ptrs, sizes, N, k, min_hits=2, steps=5)
        found = eng.last_gather_found
        path = eng.exact_gather(fixture_paths, sample_paths, k, min_hits=2, steps=5)
        assert path[1].any() and found == eng.last_gather_found
        assert all(x.tobytes() == y.tobytes() for x, y in zip(dev, path)), k
        same(path, want(k, True, 2, 5)[0], k)


# ---- 8. the argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], sample_paths[:2]
    OUT = ("pick", "unique", "depth", "shared", "total")

    def call(paths=paths, smp=smp, k=11, min_hits=1, steps=3, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        rows, cols = max(ns, 1), min(max(steps, 1), 64)
        out = {"pick": np.full((rows, cols), 77, dtype=np.int32), "unique": np.full((rows, cols), 77, dtype=np.uint64),
               "depth": np.full((rows, cols), 77, dtype=np.uint64), "shared": np.full((rows, max(n, 1)), 77, dtype=np.uint64),
               "total": np.full((rows, 2), 77, dtype=np.uint64)}
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_gather(eng._ctx, None if "paths" in null else pa, n, None if "samples" in null else sa, ns, k, min_hits, steps,
                                 *(None if name in null else out[name].ctypes.data for name in OUT),
                                 None if "found" in null else ctypes.byref(found))
        return rc, [out[name] for name in OUT], found.value, lib.dd_last_error().decode()

    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    want3 = arrays([gather_ref.answer(gs.samples()[j][2], 11, True, masks, 3) for j in range(2)])

    def usable():
        rc, out, found, _ = call()
        assert rc == 0 and found == len(masks)
        same(out, want3)
    usable()
    for kw, text in ((dict(paths=[]), "n=0 outside 1..64"), (dict(paths=paths[:1] * 65, steps=1), "n=65 outside 1..64"),
                     (dict(smp=[]), "ns=0 outside 1..1024"), (dict(smp=smp[:1] * 1025), "ns=1025 outside 1..1024"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(min_hits=0), "min_hits=0"), (dict(steps=0), "steps=0 outside 1..3"), (dict(steps=4), "steps=4 outside 1..3"),
                     (dict(steps=-1), "steps=-1 outside 1..3"),
                     *((dict(null=(name,)), "null argument") for name in OUT + ("found", "paths", "samples"))):
        rc, out, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert all((a == 77).all() for a in out) and found == 77, kw     # the outputs are untouched
        usable()
    # the rules run in the ABI comment's order: the universe's, then min_hits, then steps, then the outputs
    assert "n=0" in call(paths=[], min_hits=0, steps=0, null=("pick",))[3]
    assert "min_hits=0" in call(min_hits=0, steps=0, null=("pick",))[3]
    assert "steps=0" in call(steps=0, null=("pick",))[3]
    # ... and the device form's buffers behind them all
    def device(min_hits=1):
        out = [np.full((2, 3), 77, dtype=t) for t in (np.int32, np.uint64, np.uint64, np.uint64)] + [np.full((2, 2), 77, dtype=np.uint64)]
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_gather_device(eng._ctx, (ctypes.c_void_p * 5)(), None, 3, 2, 11, min_hits, 3, *(a.ctypes.data for a in out), ctypes.byref(found))
        return rc, out, found.value, lib.dd_last_error().decode()
    rc, out, found, err = device()
    assert rc == DD_EINVAL and "null argument" in err and all((a == 77).all() for a in out) and found == 77
    assert "min_hits=0" in device(min_hits=0)[3]
    usable()
    # a universe without a token, samples with some: nothing picked, nothing found
    z = eng.exact_gather([fixture_paths[6]], smp, 11)
    assert (z[0] == -1).all() and not any(a.any() for a in z[1:]) and eng.last_gather_found == 0
    be = HipExactBackend()
    try:
        assert be.gather_picks([[f"leaf{i}.k11"] for i in range(65)], 11, smp, 1, 3) is None
    finally:
        be.close()


# ---- 9. degenerate inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    paths, smp, fas = gs.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gs.BARREN_KS:
            got = eng.exact_gather(paths, smp, k)
            assert [a.shape for a in got] == [(3, 3), (3, 3), (3, 3), (3, 3), (3, 2)]
            assert (got[0] == -1).all() and not any(a.any() for a in got[1:]) and eng.last_gather_found == 0, (kind, canonical, k)
    dev = eng.exact_gather_device(ptrs, sizes, 3, gs.BARREN_KS[-1])
    assert eng.last_gather_found == 0 and (dev[0] == -1).all() and not any(a.any() for a in dev[1:])


def test_a_sample_that_hits_nothing(engine_factory, fixture_paths, sample_paths):
    """S3 (no byte), S4 (shorter than k) and S5 (unrelated text) alone, and in front of a sample with hits"""
    eng = engine_factory()
    k = 33
    w, _ = want(k, True)
    assert not w[4][[3, 4, 5]].any() and w[4][2].all()                    # (from the reference: the three hold no record, S2 does)
    for j in (3, 4, 5):
        got = eng.exact_gather(fixture_paths, [sample_paths[j]], k)
        assert (got[0] == -1).all() and not any(a.any() for a in got[1:]), j
    got = eng.exact_gather(fixture_paths, [sample_paths[j] for j in (3, 4, 5, 2)], k)
    same(got, [a[[3, 4, 5, 2]] for a in w])


# ---- 10. the command -----------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen --gather` on a real `--exact` tree (HipExactBackend), as a process of its own: both CSVs equal the tables
    gather_ref computes from the files' text."""
    from dandd_amd.host import deltatree
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(tmp_path), deltatree, backend=None)
    finally:
        deltatree.set_backend_factory(None)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    reads = tmp_path / "samples" / "reads.fq.gz"
    reads.write_bytes(gs.samples()[2][1])
    g = {j: b"".join(pyref.records(open(os.path.join(data, f"g{j}.fasta"), "rb").read())).decode() for j in (1, 2, 3)}
    mix = tmp_path / "samples" / "mix.fa"
    mix.write_text("".join(f">m{j}\n{r}\n" for j, r in enumerate([g[1], g[3], g[3], g[2][200:1100]])))
    order = [s["leaf"], str(mix), s["rel"], str(reads), s["far"], s["none"]]
    out = str(tmp_path / "o")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-k", "12", "-k", "33", "--gather", "--gather-min", "3",
                        "-o", out, *order], env=env, cwd=gs.ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, gs.samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = read_gather(out)
    want_tables = gather_ref.tables(universe, texts, [12, 33], min_hits=3)
    assert sorted(got) == ["gather", "gather_summary"]
    assert got["gather"] == want_tables["gather"] and got["gather_summary"] == want_tables["gather_summary"]
    assert len(got["gather_summary"]) == 6 * 2 and len([r for r in got["gather"] if r[0] == str(mix) and r[1] == "33"]) >= 3
