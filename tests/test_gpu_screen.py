"""dd_exact_screen on the MI355X: every cell of shared / match / found compared with == against Python sets of pyref.kmers over
the fixture of test_core_regions (7 inputs: an identical pair, a three-record file with N / T^70 / A^70 runs, a 40-base file, an
empty file) and seven samples -- a leaf byte for byte, a relative longer than one workgroup of segments, gzip FASTQ reads that
overlap, an empty file, one shorter than most k, unrelated text, and one record that hits the smallest and (non-canonical) the
all-ones key; the universe's own row against dd_exact_select; distinctness; 70 samples in one call; records accumulated over
passes; the argument rules; a universe that emits no record and one without a token; and `screen` end to end on a real
`--exact` tree."""
import ctypes
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_screen as cpus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [11, 28, 29, 32, 33, 60, 61, 64]     # test_gpu_core_regions': both tag modes, 64- and 128-bit keys
KS_NOCANON = [11, 32, 33, 64]
DD_EINVAL = -1
N, FULL = 7, 127


def queries(n=N, groups=cpur.GROUPS):
    """(0, 0), (full, 0), core / private / signature of every group, and a pair with all & none != 0"""
    full = (1 << n) - 1
    qs = [(0, 0), (full, 0)]
    for members in groups:
        G = sum(1 << i for i in members)
        qs.extend([(G, 0), (0, full ^ G), (G, full ^ G)])
    qs.append((3, 1))
    return qs


def fasta(text, name="s", width=70):
    return (f">{name}\n" + "".join(text[j:j + width] + "\n" for j in range(0, len(text), width))).encode()


@functools.lru_cache(maxsize=None)
def samples():
    """-> [(file name, file bytes, text whose k-mers the file holds)] S0..S6"""
    anc = np.random.default_rng(20261019).integers(0, 4, 6100)           # the ancestor of test_core_regions.genomes()
    rng = np.random.default_rng(1019)
    s = np.tile(anc, 4)[:20_000].copy()                                  # 313 segments: more than one 256-thread workgroup
    mut = rng.random(len(s)) < 0.02
    s[mut] = rng.integers(0, 4, int(mut.sum()))
    s1 = fasta("".join("ACGT"[c] for c in s), "s1")
    g1 = b"".join(pyref.records(cpur.genomes()[1])).decode()
    starts = rng.integers(0, len(g1) - 150, 400)                         # 400 x 150 over 6 kbp: every k-mer recurs
    reads = [g1[int(p):int(p) + 150] for p in starts]
    fq = "".join(f"@r{j} x\n{r}\n+\n{'I' * 150}\n" for j, r in enumerate(reads)).encode()
    once = "".join(f">r{j}\n{r}\n" for j, r in enumerate(reads)).encode()
    s5 = fasta("".join("ACGT"[c] for c in rng.integers(0, 4, 3000)), "s5")
    s6 = (">s6\n" + "A" * 70 + "N" + "T" * 70 + "R" + "C" * 70 + "\n").encode()
    g0 = cpur.genomes()[0]
    return (("s0.fa", g0, g0), ("s1.fa", s1, s1), ("s2.fq.gz", gzip.compress(fq), once), ("s3.fa", b"", b""),
            ("s4.fa", (">s4\n" + "ACGTTGCA" * 5 + "\n").encode(), (">s4\n" + "ACGTTGCA" * 5 + "\n").encode()), ("s5.fa", s5, s5),
            ("s6.fa", s6, s6))


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("screen_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen_samples")
    paths = []
    for name, raw, _ in samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


@functools.lru_cache(maxsize=None)
def want(k, canonical):
    """-> (shared [ns+1][n], match [ns+1][nq], found) from the sets: a computation of its own, never changed"""
    _, masks = cpur.reference(k, canonical)
    sets = [set(pyref.kmers(text, k, canonical)) for _, _, text in samples()] + [set(masks)]
    shared = [[sum(1 for x in q if masks.get(x, 0) >> i & 1) for i in range(N)] for q in sets]
    match = [[sum(1 for x in q if x in masks and masks[x] & a == a and masks[x] & b == 0) for a, b in queries()] for q in sets]
    return np.array(shared, dtype=np.uint64), np.array(match, dtype=np.uint64), len(masks)


# ---- 1. every cell against the sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in KS] + [(False, k) for k in KS_NOCANON])
def test_every_cell_equals_the_sets(engine_factory, fixture_paths, sample_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    qs = queries()
    al, no = [a for a, _ in qs], [b for _, b in qs]
    shared, match = eng.exact_screen(fixture_paths, sample_paths, k, al, no)
    assert eng.last_sketch_stats()[2] == 1
    w_shared, w_match, w_found = want(k, canonical)
    assert shared.dtype == np.uint64 and match.dtype == np.uint64
    assert shared.shape == (8, N) and match.shape == (8, len(qs))
    assert eng.last_screen_found == w_found
    assert shared.tolist() == w_shared.tolist(), (k, canonical)
    assert match.tolist() == w_match.tolist(), (k, canonical)
    # the universe's own row is what dd_exact_select counts
    own = eng.exact_select(fixture_paths, k, k, [1 << i for i in range(N)] + al, [0] * N + no)[:, 0]
    assert shared[7].tolist() == own[:N].tolist() and match[7].tolist() == own[N:].tolist()
    # the fixture does what it is for: S0 is g0 (and g4), the (all & none) pair matches nothing, S6 reaches both ends of the set
    assert shared[0, 0] == shared[7, 0] == shared[0, 4] and not match[:, -1].any() and not shared[3].any()
    _, masks = cpur.reference(k, canonical)
    s6 = set(pyref.kmers(samples()[6][2], k, canonical))
    assert min(masks) == 0 and 0 in s6
    if not canonical:
        assert max(masks) == (1 << 2 * k) - 1 and max(masks) in s6
    assert match[6, 0] >= (1 if canonical else 2)


# ---- 2. distinctness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_repeats_count_once(engine_factory, fixture_paths, sample_paths, tmp_path, k):
    eng = engine_factory()
    _, raw, once = samples()[2]
    (tmp_path / "once.fa").write_bytes(once)
    (tmp_path / "thrice.fq.gz").write_bytes(raw * 3)                     # three gzip members
    qs = queries()
    shared, match = eng.exact_screen(fixture_paths, [sample_paths[2], str(tmp_path / "once.fa"), str(tmp_path / "thrice.fq.gz")], k,
                                     [a for a, _ in qs], [b for _, b in qs])
    w_shared, w_match, _ = want(k, True)
    for row in range(3):
        assert shared[row].tolist() == w_shared[2].tolist() and match[row].tolist() == w_match[2].tolist(), row
    assert shared[0, 1] > 0 and shared[0, 1] < 400 * (150 - k + 1)        # far fewer distinct k-mers than occurrences


# ---- 3. many samples, one call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 61])
def test_seventy_samples_in_one_call(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    qs = queries()
    al, no = [a for a, _ in qs], [b for _, b in qs]
    many = [sample_paths[j % 7] for j in range(70)]
    shared, match = eng.exact_screen(fixture_paths, many, k, al, no)
    found = eng.last_screen_found
    assert shared.shape == (71, N) and match.shape == (71, len(qs))
    for j in range(7):
        one_s, one_m = eng.exact_screen(fixture_paths, [sample_paths[j]], k, al, no)
        assert eng.last_screen_found == found
        assert one_s[1].tolist() == shared[70].tolist() and one_m[1].tolist() == match[70].tolist()
        for row in range(j, 70, 7):
            assert shared[row].tolist() == one_s[0].tolist() and match[row].tolist() == one_m[0].tolist(), (k, row)
    w_shared, w_match, _ = want(k, True)
    assert shared[:7].tolist() == w_shared[:7].tolist() and match[70].tolist() == w_match[7].tolist()


# ---- 4. records accumulated over passes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 31, 62])
def test_multi_pass_gives_identical_counts(engine_factory, tmp_path, k):
    """The 17 x 19 kbp universe of test_gpu_core_regions' G4 with a 1 MiB sort budget: at least three passes append their
    records before the one ordering the samples are looked up in."""
    eng = engine_factory()
    family = greedy.related(18, 19_000, 17)                               # (the first 17 are G4's; the 18th is a relative outside)
    paths = greedy.write(tmp_path, family[:17])
    other = greedy.write(tmp_path, family[17:], tag="x")
    full = (1 << 17) - 1
    qs = [(0, 0), (full, 0), (0b111, 0), (0, full ^ 0b111), (1 << 5, full ^ (1 << 5))]
    al, no = [a for a, _ in qs], [b for _, b in qs]
    smp = [paths[5], other[0]]
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_screen(paths, smp, k, al, no)
    found = eng.last_screen_found
    assert eng.last_sketch_stats()[2] == 1
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = eng.exact_screen(paths, smp, k, al, no)
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_screen_found > 65_536
    assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes()
    shared, match = one
    assert 0 < shared[0, 5] == shared[2, 5] == match[0, 0]                 # a genome of the universe: all of it is there
    assert match[2, 0] == found and shared[0].all() and 0 < match[1, 0] < match[0, 0]


# ---- 5. the argument rules -------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], sample_paths[:2]

    def call(paths=paths, smp=smp, k=11, al=(1, 0), no=(0, 6), nq=None, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        nq = len(al) if nq is None else nq
        a, b = np.array(list(al) or [0], dtype=np.uint64), np.array(list(no) or [0], dtype=np.uint64)
        shared = np.full((max(ns, 0) + 1, max(n, 1)), 77, dtype=np.uint64)
        match = np.full((max(ns, 0) + 1, max(nq, 1)), 77, dtype=np.uint64)
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_screen(eng._ctx, pa, n, sa, ns, k, None if "all" in null else a.ctypes.data, None if "none" in null else b.ctypes.data,
                                 nq, None if "shared" in null else shared.ctypes.data, None if "match" in null else match.ctypes.data,
                                 ctypes.byref(found))
        return rc, shared, match, found.value, lib.dd_last_error().decode()

    def usable():
        rc, shared, match, found, _ = call()
        assert rc == 0 and found == want3[2] and shared.tolist() == want3[0] and match.tolist() == want3[1]
    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    sets = [set(pyref.kmers(samples()[j][2], 11)) for j in range(2)] + [set(masks)]
    want3 = ([[sum(1 for x in q if masks.get(x, 0) >> i & 1) for i in range(3)] for q in sets],
             [[sum(1 for x in q if x in masks and masks[x] & a == a and masks[x] & b == 0) for a, b in ((1, 0), (0, 6))] for q in sets], len(masks))
    usable()
    for kw, text in ((dict(paths=[]), "n=0 outside 1..64"), (dict(paths=paths[:1] * 65), "n=65 outside 1..64"),
                     (dict(smp=[]), "ns=0 outside 1..1024"), (dict(smp=smp[:1] * 1025), "ns=1025 outside 1..1024"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(al=(1, 8)), "query 1: a bit outside 0..2"), (dict(no=(0, 1 << 63)), "query 1: a bit outside 0..2"),
                     (dict(al=(1,) * 1025, no=(0,) * 1025), "nq=1025 outside 0..1024"), (dict(nq=-1), "nq=-1 outside 0..1024"),
                     (dict(null=("shared",)), "null argument"), (dict(null=("match",)), "null argument"),
                     (dict(null=("all",)), "null argument")):
        rc, shared, match, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert (shared == 77).all() and (match == 77).all() and found == 77, kw     # the outputs are untouched
        usable()
    # nq == 0: all, none and match may be null
    rc, shared, match, found, _ = call(al=(), no=(), nq=0, null=("all", "none", "match"))
    assert rc == 0 and shared.tolist() == want3[0] and found == want3[2] and (match == 77).all()
    got = eng.exact_screen(paths, smp, 11, [], [])
    assert got[0].tolist() == want3[0] and got[1].shape == (3, 0)
    # 1024 queries; two calls, identical bytes
    big = eng.exact_screen(paths, smp, 11, [1, 0] * 512, [0, 6] * 512)
    assert big[1].tolist() == [row * 512 for row in want3[1]]
    qs = queries(3, [[0, 1], [2]])
    a = eng.exact_screen(paths, sample_paths, 33, [x for x, _ in qs], [y for _, y in qs])
    b = eng.exact_screen(paths, sample_paths, 33, [x for x, _ in qs], [y for _, y in qs])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].any()
    # a universe without a token, samples with some: zero rows, nothing found
    z = eng.exact_screen([fixture_paths[6]], smp, 11, [0], [0])
    assert not z[0].any() and not z[1].any() and eng.last_screen_found == 0
    be = HipExactBackend()
    try:
        assert be.screen_counts([[f"leaf{i}.k11"] for i in range(65)], 11, smp, [0], [0]) is None
    finally:
        be.close()


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = samples()[2][2]
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    qs = queries()
    al, no = [a for a, _ in qs], [b for _, b in qs]
    for k in (21, 62):
        dev, path = eng.exact_screen_device(ptrs, sizes, N, k, al, no), eng.exact_screen(fixture_paths, sample_paths, k, al, no)
        assert path[0].any() and dev[0].tolist() == path[0].tolist() and dev[1].tolist() == path[1].tolist(), k


# ---- 6. a universe that leaves the emission nothing ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def barren():
    """-> {name: three universe files}: one 20-base record each (tokens, but no k-mer at k = 21 or 33: the emission runs and
    finds no record), and 0 bytes each (no token: no emission at all)"""
    rng = np.random.default_rng(2133)
    short = tuple(fasta("".join("ACGT"[c] for c in rng.integers(0, 4, 20)), f"u{i}") for i in range(3))
    assert all(cpur.index_of(fa)[2] == 21 for fa in short)
    return {"no record": short, "no token": (b"", b"", b"")}


BARREN_SAMPLES = (0, 3, 4)                                               # a leaf of the big fixture, the empty file, 40 bases
BARREN_KS = (21, 33)


def barren_files(tmp_path, kind):
    """-> (universe paths, sample paths, the texts of both in the device forms' order)"""
    fas = list(barren()[kind]) + [samples()[j][1] for j in BARREN_SAMPLES]
    paths = greedy.write(tmp_path, fas[:3]) + greedy.write(tmp_path, fas[3:], tag="s")
    return paths[:3], paths[3:], fas


def on_device(torch, fas):
    """-> (the tensors, their addresses, the texts' sizes): each text with 16 bytes behind it, as the device forms ask"""
    bufs = [torch.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    return bufs, [b.data_ptr() for b in bufs], [len(f) for f in fas]


@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    paths, smp, fas = barren_files(tmp_path, kind)
    bufs, ptrs, sizes = on_device(torch_cuda, fas)
    al, no = [0, 7, 1], [0, 0, 6]
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in BARREN_KS:
            shared, match = eng.exact_screen(paths, smp, k, al, no)
            assert shared.shape == (4, 3) and match.shape == (4, 3)
            assert not shared.any() and not match.any() and eng.last_screen_found == 0, (kind, canonical, k)
    dev = eng.exact_screen_device(ptrs, sizes, 3, BARREN_KS[-1], al, no)
    assert eng.last_screen_found == 0 and dev[0].tolist() == shared.tolist() and dev[1].tolist() == match.tolist()


# ---- 7. the command -----------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen` on a real `--exact` tree (HipExactBackend), as a process of its own: the three CSVs equal the tables
    test_screen computes from the files' text."""
    from dandd_amd.host import deltatree
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(tmp_path), deltatree, backend=None)
    finally:
        deltatree.set_backend_factory(None)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    s = cpus.make_samples(tmp_path, data)
    reads = tmp_path / "samples" / "reads.fq.gz"
    reads.write_bytes(samples()[2][1])
    order = [s["leaf"], s["rel"], str(reads), s["far"], s["none"]]
    out = str(tmp_path / "o")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-g", gfile, "-k", "9", "-k", "12", "-k", "33",
                        "-o", out, *order], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = cpus.read_csvs(out)
    assert got == cpus.tables(universe, texts, [9, 12, 33], groups)
    assert len(got["screen"]) == 5 * 3 * 5
