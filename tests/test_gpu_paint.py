"""dd_exact_paint on the MI355X: every cell of every window compared with == against paint_ref (k-mer ends and masks from
Python dictionaries) over the fixture of test_core_regions and the seven samples of test_gpu_screen, at window sizes that take
each way out of the kernel (one segment, a border inside a wave, a whole wave, one window for a whole sample); a 64-input
universe whose shared stretch carries every counter into the top plane and sets bit 63; window sums across wave and workgroup
borders; passes and determinism; 70 samples in one call and the device form; the argument rules; and `screen --paint` end to
end on a real `--exact` tree."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import paint_ref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_gpu_screen as gpus
import test_paint as cpup
import test_screen as cpus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = gpus.KS
KS_NOCANON = gpus.KS_NOCANON
DD_EINVAL = -1
N = 7
WINDOWS = (64, 192, 4096, 60416)      # one segment; no power of two; one whole wave; larger than every sample (S2: 60 400 tokens)


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("paint_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("paint_samples")
    paths = []
    for name, raw, _ in gpus.samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


@functools.lru_cache(maxsize=None)
def sample_ends(j, k, canonical):
    return cpur.ends_of(gpus.samples()[j][2], k, canonical)


@functools.lru_cache(maxsize=None)
def want(j, k, canonical, window):
    """the rows of sample j from paint_ref: a computation of its own, never changed"""
    _, masks = cpur.reference(k, canonical)
    return paint_ref.rows(gpus.samples()[j][2], k, canonical, masks, N, window, ends=sample_ends(j, k, canonical))


def ntoks():
    return [cpur.index_of(text)[2] for _, _, text in gpus.samples()]


# ---- 1. every cell against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in KS] + [(False, k) for k in KS_NOCANON])
def test_every_cell_equals_the_reference(engine_factory, fixture_paths, sample_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    nt = ntoks()
    assert nt[3] == 0 and nt[4] == 41 and nt[1] == 20_001 and max(nt) == nt[2] == 60_400 < WINDOWS[-1]
    for window in WINDOWS:
        got = eng.exact_paint(fixture_paths, sample_paths, k, window, ntok=nt if window != 192 else None)
        assert eng.last_sketch_stats()[2] == 1 and eng.last_paint_found == len(cpur.reference(k, canonical)[1])
        assert len(got) == 7
        for j, rows in enumerate(got):
            assert rows.dtype == np.uint32 and rows.shape == (-(-nt[j] // window), N + 2), (j, window)
            assert rows.tolist() == want(j, k, canonical, window), (k, canonical, window, j)
        # S0 is g0 (and g4) byte for byte: every valid position is in the universe, in g0 and in g4
        s0 = got[0]
        assert s0[:, 0].sum() == 6000 - k + 1
        assert (s0[:, 0] == s0[:, 1]).all() and (s0[:, 0] == s0[:, 2 + 0]).all() and (s0[:, 0] == s0[:, 2 + 4]).all()
        # the empty sample has no rows; the one of 40 bases has one row, all zero from k = 41 on
        assert got[3].shape == (0, N + 2) and got[4].shape == (1, N + 2)
        assert got[4][0, 0] == max(0, 40 - k + 1) and (k <= 40 or not got[4].any())
        if window == WINDOWS[-1]:
            assert all(len(rows) == (1 if nt[j] else 0) for j, rows in enumerate(got))
            assert not got[5][:, 1:].any() or k < 16              # unrelated text: nothing of it in the universe
    # the positions the universe holds are no fewer than the distinct k-mers screen counts
    shared, _ = eng.exact_screen(fixture_paths, sample_paths, k, [], [])
    total = np.array([rows.sum(axis=0) for rows in got], dtype=np.uint64)
    assert (total[:, 2:] >= shared[:7]).all() and (total[2, 2:] > shared[2]).any()      # (the reads of S2 overlap)


# ---- 2. all seven planes and bit 63 -------------------------------------------------------------------------------------------
STRETCH_AT = 1050     # where the shared stretch starts in the 4 kbp input: the tokens 1 + 1050 + 32 .. 1 + 1050 + 199 end a
#                       k-mer of it at k = 33, which holds the segment of the tokens 1088 .. 1151 whole (and 1152 .. 1215)


@functools.lru_cache(maxsize=None)
def wide_universe():
    """64 inputs: 0..62 mutants of a 300-base ancestor, 63 a 4 kbp file; a stretch of 200 random bases stands in every one"""
    rng = np.random.default_rng(63)
    text = lambda codes: "".join("ACGT"[c] for c in codes)
    stretch = text(rng.integers(0, 4, 200))
    anc = rng.integers(0, 4, 100)
    fas = []
    for i in range(63):
        s = anc.copy()
        mut = rng.random(100) < 0.05
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        fas.append(gpus.fasta(text(s[:50]) + stretch + text(s[50:]), f"m{i}"))
    big = text(rng.integers(0, 4, 4000))
    fas.append(gpus.fasta(big[:STRETCH_AT] + stretch + big[STRETCH_AT + 200:], "big"))
    return tuple(fas)


@functools.lru_cache(maxsize=None)
def wide_want(k, window):
    fas = wide_universe()
    masks = {}
    for i, fa in enumerate(fas):
        for x in cpur.ends_of(fa, k, True).values():
            masks[x] = masks.get(x, 0) | 1 << i
    return paint_ref.rows(fas[63], k, True, masks, 64, window), len(masks)


def test_the_reference_of_the_wide_universe_fills_a_segment():
    """(no GPU work: the fixture does what it is for) a W = 64 row of the reference is 64 in all 66 columns at both ks"""
    for k in (11, 33):
        rows, _ = wide_want(k, 64)
        assert [64] * 66 in rows, k
        assert max(max(r) for r in rows) == 64


@pytest.mark.parametrize("k", [11, 33])
def test_all_seven_planes_and_bit_63(engine_factory, tmp_path, k):
    eng = engine_factory()
    paths = greedy.write(tmp_path, wide_universe())
    for window in (64, 192, 4096):
        rows, found = wide_want(k, window)
        got = eng.exact_paint(paths, [paths[63]], k, window)
        assert eng.last_paint_found == found
        assert got[0].shape == (-(-4001 // window), 66) and got[0].tolist() == rows, (k, window)
        if window == 64:
            full = [i for i, r in enumerate(got[0].tolist()) if r == [64] * 66]
            assert full and (1 + STRETCH_AT + 199) // 64 - 1 in full             # the carry into the top plane, in every column
            assert (got[0][:, 2 + 63] == got[0][:, 0]).all()                      # the sample is input 63: bit 63 at every position


# ---- 3. window and wave borders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_wide_windows_are_sums_of_the_segments(engine_factory, fixture_paths, sample_paths, k):
    """S1: 20 001 tokens, 313 segments, two workgroups, five waves"""
    eng = engine_factory()
    one = eng.exact_paint(fixture_paths, [sample_paths[1]], k, 64)[0].astype(np.uint64)
    assert one.shape == (313, N + 2) and one.tolist() == want(1, k, True, 64)
    for window in (4096, 8192, 1 << 22):
        got = eng.exact_paint(fixture_paths, [sample_paths[1]], k, window)[0]
        per = window // 64
        sums = [one[w * per:(w + 1) * per].sum(axis=0).tolist() for w in range(-(-313 // per))]
        assert got.tolist() == sums, (k, window)
        assert got.tolist() == want(1, k, True, window), (k, window)
    assert got.shape == (1, N + 2) and got[0].tolist() == one.sum(axis=0).tolist()


# ---- 4. passes and determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 62])
def test_multi_pass_gives_identical_bytes(engine_factory, tmp_path, k):
    """test_gpu_screen's 17 x 19 kbp universe with a 1 MiB sort budget: at least three passes append their records before the
    one ordering the samples are looked up in."""
    eng = engine_factory()
    family = greedy.related(18, 19_000, 17)
    paths = greedy.write(tmp_path, family[:17])
    other = greedy.write(tmp_path, family[17:], tag="x")
    smp = [paths[5], other[0]]
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_paint(paths, smp, k, 4096)
    found = eng.last_paint_found
    assert eng.last_sketch_stats()[2] == 1
    again = eng.exact_paint(paths, smp, k, 4096)
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = eng.exact_paint(paths, smp, k, 4096)
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_paint_found > 65_536
    for a, b, c in zip(one, again, many):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    # a genome of the universe: every position is there, and in itself; a relative outside: some are, not all
    assert one[0][:, 0].sum() == 19_000 - k + 1 and (one[0][:, 0] == one[0][:, 2 + 5]).all()
    assert 0 < one[1][:, 1].sum() < one[1][:, 0].sum()


# ---- 5. many samples, one call; the device form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 61])
def test_seventy_samples_in_one_call(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    nt = ntoks()
    many = eng.exact_paint(fixture_paths, [sample_paths[j % 7] for j in range(70)], k, 192, ntok=[nt[j % 7] for j in range(70)])
    found = eng.last_paint_found
    assert len(many) == 70
    for j in range(7):
        one = eng.exact_paint(fixture_paths, [sample_paths[j]], k, 192, ntok=[nt[j]])[0]
        assert eng.last_paint_found == found and one.tolist() == want(j, k, True, 192)
        for row in range(j, 70, 7):
            assert many[row].tobytes() == one.tobytes() and many[row].shape == one.shape, (k, row)


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = gpus.samples()[2][2]
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    nt = ntoks()
    for k, window in ((21, 64), (62, 4096)):
        dev, path = eng.exact_paint_device(ptrs, sizes, N, k, window, nt), eng.exact_paint(fixture_paths, sample_paths, k, window)
        assert len(dev) == len(path) == 7 and path[0].any()
        assert all(d.tobytes() == p.tobytes() and d.shape == p.shape for d, p in zip(dev, path)), k


@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    """test_gpu_screen's barren universes: column 0 is the sample's own, every other column is zero.  Without a token in the
    universe no emission stages the table of the samples' first rows: the entry does."""
    paths, smp, fas = gpus.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gpus.on_device(torch_cuda, fas)
    texts = [gpus.samples()[j][2] for j in gpus.BARREN_SAMPLES]
    nt = [cpur.index_of(text)[2] for text in texts]
    assert nt == [6001, 0, 41]
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gpus.BARREN_KS:
            for window in (64, 4096):
                got = eng.exact_paint(paths, smp, k, window, ntok=nt)
                assert eng.last_paint_found == 0 and len(got) == 3
                for text, rows in zip(texts, got):
                    want = paint_ref.rows(text, k, canonical, {}, 3, window)
                    assert rows.shape == (len(want), 5) and rows[:, 0].tolist() == [w[0] for w in want], (kind, canonical, k, window)
                    assert not rows[:, 1:].any()
                assert got[0][:, 0].sum() == 6000 - k + 1
    dev = eng.exact_paint_device(ptrs, sizes, 3, k, window, nt)
    assert eng.last_paint_found == 0 and len(dev) == 3
    assert all(d.tolist() == p.tolist() and d.shape == p.shape for d, p in zip(dev, got))


# ---- 6. the argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], sample_paths[:2]
    nt = ntoks()[:2]
    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    want3 = [paint_ref.rows(gpus.samples()[j][2], 11, True, masks, 3, 192) for j in range(2)]
    spans = [len(w) for w in want3]

    def call(paths=paths, smp=smp, k=11, window=192, spans=spans, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        off = np.zeros(max(ns, 0) + 1, dtype=np.uint64)
        off[1:1 + len(spans)] = np.cumsum(spans[:ns], dtype=np.uint64) if ns else []
        counts = np.full((max(int(off[-1]), 1) + 1, min(n, 64) + 2), 77, dtype=np.uint32)
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_paint(eng._ctx, pa, n, sa, ns, k, window, None if "off" in null else off.ctypes.data,
                                None if "counts" in null else counts.ctypes.data, ctypes.byref(found))
        return rc, counts, found.value, lib.dd_last_error().decode()

    def usable():
        rc, counts, found, _ = call()
        assert rc == 0 and found == len(masks) and counts[:-1].tolist() == want3[0] + want3[1] and (counts[-1] == 77).all()
    usable()
    top = (1 << 22) + 64
    for kw, text in ((dict(window=0), "window=0: a multiple of 64 in 64..4194304"), (dict(window=63), "window=63: a multiple of 64"),
                     (dict(window=65), "window=65: a multiple of 64"), (dict(window=top), f"window={top}: a multiple of 64 in 64..4194304"),
                     (dict(spans=[spans[0], spans[1] + 1]), f"sample 1: off[2] - off[1] = {spans[1] + 1} rows, {spans[1]} expected"),
                     (dict(spans=[spans[0] - 1, spans[1]]), f"sample 0: off[1] - off[0] = {spans[0] - 1} rows, {spans[0]} expected"),
                     (dict(smp=[], spans=[]), "ns=0 outside 1..1024"), (dict(smp=smp[:1] * 1025, spans=[spans[0]] * 1025), "ns=1025 outside 1..1024"),
                     (dict(paths=paths[:1] * 65), "n=65 outside 1..64"), (dict(paths=[]), "n=0 outside 1..64"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(null=("counts",)), "null argument"), (dict(null=("off",)), "null argument")):
        rc, counts, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert (counts == 77).all() and found == 77, kw                      # the outputs are untouched
        usable()
    assert f"{nt[1]} tokens" in call(spans=[spans[0], spans[1] + 1])[3]
    # no row asked for: counts may be null (an empty sample, and one more)
    rc, _, found, err = call(smp=[sample_paths[3]] * 2, spans=[0, 0], null=("counts",))
    assert rc == 0 and found == len(masks), err
    # a universe without a token: column 0 alone
    z = eng.exact_paint([fixture_paths[6]], smp, 11, 192)
    assert eng.last_paint_found == 0 and [r[:, 0].tolist() for r in z] == [[row[0] for row in w] for w in want3]
    assert not any(r[:, 1:].any() for r in z)
    be = HipExactBackend()
    try:
        assert be.paint_counts([[f"leaf{i}.k11"] for i in range(65)], 11, smp, 192) is None
    finally:
        be.close()


# ---- 7. the command ------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen --paint 192` on a real `--exact` tree (HipExactBackend), as processes of their own: paint.csv equals the table
    paint_ref computes from the files' text, the screen files are what they are without --paint."""
    from dandd_amd.host import deltatree
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(tmp_path), deltatree, backend=None)
    finally:
        deltatree.set_backend_factory(None)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    reads = tmp_path / "samples" / "reads.fq.gz"
    reads.write_bytes(gpus.samples()[2][1])
    order = [s["leaf"], s["rel"], cpup._mosaic(tmp_path, data), str(reads), s["far"], s["none"]]
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    outs = {}
    for name, extra in (("plain", []), ("paint", ["--paint", "192", "--paint-matrix"])):
        outs[name] = str(tmp_path / name)
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-k", "12", "-k", "33", "-o", outs[name], *extra,
                            *order], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, gpus.samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = cpup.read_paint(outs["paint"], [name for name, _ in universe])
    want = paint_ref.tables(universe, texts, [12, 33], 192)
    assert sorted(got) == ["paint", "paint_matrix", "paint_segments"]
    for name in want:
        assert got[name] == want[name], name
    assert not cpup.read_paint(outs["plain"], []) and len(got["paint"]) > 200
    before, after = cpus.read_csvs(outs["plain"]), cpus.read_csvs(outs["paint"])
    assert sorted(before) == ["screen", "screen_summary"] and before == after
    for name in before:
        path = f"gold_5_kmc.{name}.csv"
        assert open(os.path.join(outs["plain"], path), "rb").read() == open(os.path.join(outs["paint"], path), "rb").read()
