"""dd_exact_cover on the MI355X: every cell of the six columns compared with == against cover_ref (a target's k-mer ends, the
sample's depths from a collections.Counter, binned in plain Python) over test_core_regions' universe and test_gpu_screen's
samples, in both strand modes, at windows that take each of the kernel's three ways to a row and at three clips; the
identities with dd_exact_locate and between windows; a counter past 16 bits under the clip; more than one workgroup, window
borders inside a wave and records accumulated over passes; samples taken in rounds; two calls byte for byte; the device form;
the argument rules; degenerate inputs; and `screen --cover` end to end on a real `--exact` tree."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_ref
import depth_ref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_gpu_screen as gs
import test_screen as cpus
from test_cover import read_cover

pytestmark = pytest.mark.gpu

N = gs.N
DD_EINVAL = -1
CLIPS = (1, 3, 1023)
NTOK = [cpur.index_of(fa)[2] for fa in cpur.genomes()]


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("cover_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("cover_samples")
    paths = []
    for name, raw, _ in gs.samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


@functools.lru_cache(maxsize=None)
def depth_of(s, k, canonical):
    return depth_ref.depths(gs.samples()[s][2], k, canonical, cpur.reference(k, canonical)[1])


@functools.lru_cache(maxsize=None)
def want(k, canonical, window, clip):
    """-> per target g of the fixture a uint32 [7][nwin_g][6] array of S0..S6 from cover_ref: a computation of its own, never changed"""
    ends, masks = cpur.reference(k, canonical)
    return [np.array([cover_ref.rows(ends[g], g, NTOK[g], depth_of(s, k, canonical), masks, window, clip) for s in range(7)],
                     dtype=np.uint32).reshape(7, -(-NTOK[g] // window), 6) for g in range(N)]


def same(got, wanted, why):
    assert len(got) == len(wanted)
    for g, (a, b) in enumerate(zip(got, wanted)):
        assert a.dtype == np.uint32 and a.shape == b.shape, (why, g, a.shape, b.shape)
        assert a.tolist() == b.tolist(), (why, g)


# ---- 1. every cell against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in gs.KS] + [(False, k) for k in gs.KS_NOCANON])
def test_every_cell_equals_the_reference(engine_factory, fixture_paths, sample_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    assert NTOK[1] == 64 * 94 and NTOK[2] == 64 * 94 + 1 and NTOK[5] == 41 and NTOK[6] == 0
    for window in (64, 192, 4096) if k in (29, 33) else (64,):
        for clip in CLIPS:
            got = eng.exact_cover(fixture_paths, sample_paths, k, window, clip=clip)
            assert eng.last_sketch_stats()[2] == 1 and eng.last_cover_found == len(cpur.reference(k, canonical)[1])
            same(got, want(k, canonical, window, clip), (k, canonical, window, clip))
            assert got[6].shape == (7, 0, 6) and got[5].shape == (7, 1, 6)          # g6 owns no rows
            if window == 4096:
                assert got[1].shape == (7, 2, 6) and got[2].shape == (7, 2, 6)       # the whole-wave path, two windows
    # the fixture does what it is for
    w3, w1023 = want(k, canonical, 64, 3), want(k, canonical, 64, 1023)
    allw = np.concatenate(w3, axis=1).astype(np.int64)
    assert ((allw[..., 1] > 0) & (allw[..., 1] < allw[..., 0])).any()                  # a window that is partly covered
    assert (np.concatenate(w1023, axis=1)[..., 2] > np.concatenate(w3, axis=1)[..., 2]).any()   # a cell clipped at 3 and not at 1023
    assert (allw[..., 4] > 0).any()                                                  # a private position that a sample holds
    assert not w3[0][..., 3:].any() and not w3[4][..., 3:].any() and w3[0][..., 0].any()   # g0 = g4: neither has a private position
    assert w3[1][..., 3].any() and w3[3][..., 3].any()


# ---- 2. identities with entry points that exist ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 61])
def test_identities(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    full = (1 << N) - 1
    c64 = eng.exact_cover(fixture_paths, sample_paths, k, 64, clip=255, ntok=NTOK)
    found = eng.last_cover_found
    jobs = [(0, 0, g) for g in range(N)] + [(1 << g, full ^ (1 << g), g) for g in range(N)]
    hits = eng.exact_locate(fixture_paths, k, jobs, ntok=NTOK)
    assert eng.last_locate_found == found
    pop = lambda words: int(np.unpackbits(words.view(np.uint8)).sum())
    for g in range(N):
        for s in range(7):
            assert int(c64[g][s, :, 0].sum()) == pop(hits[g]) and int(c64[g][s, :, 3].sum()) == pop(hits[N + g]), (g, s)
    assert pop(hits[1]) > 5000 and pop(hits[N + 1]) > 0
    # clip = 1: depth is covered, byte for byte
    c1 = eng.exact_cover(fixture_paths, sample_paths, k, 64, clip=1)
    for g in range(N):
        assert c1[g][..., 2].tobytes() == c1[g][..., 1].tobytes() and c1[g][..., 5].tobytes() == c1[g][..., 4].tobytes()
        assert c1[g][..., [0, 1, 3, 4]].tobytes() == c64[g][..., [0, 1, 3, 4]].tobytes()
    # S0 is g0 (and g4) byte for byte: it covers every position of both
    for g in (0, 4):
        assert c64[g][0, :, 1].tolist() == c64[g][0, :, 0].tolist() and c64[g][0, :, 0].sum() > 5000
    # a window of 128 is two of 64
    c128 = eng.exact_cover(fixture_paths, sample_paths, k, 128, clip=255)
    for g in range(N):
        a = c64[g].astype(np.uint64)
        if a.shape[1] % 2:
            a = np.concatenate([a, np.zeros((7, 1, 6), dtype=np.uint64)], axis=1)
        assert c128[g].astype(np.uint64).tolist() == (a[:, 0::2] + a[:, 1::2]).tolist(), g
    # S3 (empty) and S4 (shorter than k, or nothing of the universe): the sample-independent columns alone
    for g in range(N):
        for s in (3, 4):
            assert not c64[g][s][:, [1, 2, 4, 5]].any()
        for s in range(1, 7):
            assert c64[g][s][:, [0, 3]].tobytes() == c64[g][0][:, [0, 3]].tobytes()


# ---- 3. a counter past 16 bits under the clip --------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, 21), (True, 33), (False, 64)])
def test_a_counter_past_sixteen_bits(engine_factory, fixture_paths, tmp_path, canonical, k):
    eng = engine_factory(canonical=canonical)
    text = (">poly\n" + "A" * 70_000 + "\n").encode()
    path = tmp_path / "poly.fa"
    path.write_bytes(text)
    ends, masks = cpur.reference(k, canonical)
    assert masks[0] == 1 << 3                                            # A^k is a record of the universe, and g3's alone
    depth = depth_ref.depths(text, k, canonical, masks)
    assert depth == {0: 70_001 - k} and depth[0] > 1 << 16
    runs = 2 if canonical else 1                                         # canonical: g3's T^70 run is the same record
    places = sum(1 for x in ends[3].values() if x == 0)                  # (a run is 70 bases, or a base more where its neighbour agrees)
    assert runs * (70 - k + 1) <= places <= runs * (72 - k + 1)
    for clip in (1023, 7):
        got = eng.exact_cover(fixture_paths, [str(path)], k, 64, targets=[3], clip=clip, ntok=NTOK)
        assert len(got) == 1 and got[0].shape == (1, -(-NTOK[3] // 64), 6)
        assert got[0][0].tolist() == cover_ref.fixture_rows(3, text, k, canonical, 64, clip)
        rows = got[0][0].astype(np.int64)
        assert rows[:, 1].sum() == places and rows[:, 2].tolist() == (clip * rows[:, 1]).tolist()
        assert rows[:, 4].tolist() == rows[:, 1].tolist() and rows[:, 5].tolist() == rows[:, 2].tolist()      # private to g3


# ---- 4. more than one workgroup, borders that are not wave-aligned, several passes --------------------------------------------
@functools.lru_cache(maxsize=None)
def family():
    return tuple(greedy.related(18, 19_000, 17))


@functools.lru_cache(maxsize=None)
def family_reference(k):
    """-> ([{end token: key}] of the 17 genomes, {key: mask}, [{key: depth}] of the two samples)"""
    fas = family()
    ends = [cpur.ends_of(fa, k, True) for fa in fas[:17]]
    masks = {}
    for i, e in enumerate(ends):
        for x in e.values():
            masks[x] = masks.get(x, 0) | 1 << i
    return ends, masks, [depth_ref.depths(fa, k, True, masks) for fa in (fas[5], fas[17])]


@pytest.mark.parametrize("k", [13, 62])
def test_multi_pass_and_window_borders(engine_factory, tmp_path, k):
    eng = engine_factory()
    fas = family()
    paths = greedy.write(tmp_path, fas[:17])
    other = greedy.write(tmp_path, fas[17:], tag="x")
    smp, targets = [paths[5], other[0]], [5, 0, 16]
    ntok = [cpur.index_of(fa)[2] for fa in fas[:17]]
    assert all(-(-t // 64) == 297 for t in ntok)                         # two workgroups of segments a genome, the second partly filled
    assert "DD_EXACT_MB" not in os.environ
    for window in (320, 4096, 1 << 22):
        one = eng.exact_cover(paths, smp, k, window, targets=targets, clip=255, ntok=ntok)
        found = eng.last_cover_found
        assert eng.last_sketch_stats()[2] == 1
        os.environ["DD_EXACT_MB"] = "1"
        try:
            many = eng.exact_cover(paths, smp, k, window, targets=targets, clip=255, ntok=ntok)
            passes = eng.last_sketch_stats()[2]
        finally:
            del os.environ["DD_EXACT_MB"]
        assert passes >= 3, (k, passes)
        assert found == eng.last_cover_found > 65_536
        for a, b in zip(one, many):
            assert a.shape == (2, -(-ntok[0] // window), 6) and a.tobytes() == b.tobytes(), (k, window)
        if window == 320:
            ends, masks, depths = family_reference(k)
            for a, g in zip(one, targets):
                assert a.tolist() == [cover_ref.rows(ends[g], g, ntok[g], d, masks, window, 255) for d in depths], (k, g)
        if window == 1 << 22:
            assert one[0][0, 0, 1] == one[0][0, 0, 0] > 18_000 and 0 < one[0][1, 0, 1] < one[0][1, 0, 0]     # genome 5 along itself; the relative


# ---- 5. samples taken in rounds ---------------------------------------------------------------------------------------------
def test_seventy_samples_in_rounds(engine_factory, fixture_paths, sample_paths):
    eng = engine_factory()
    k = 33
    many = [sample_paths[j % 7] for j in range(70)]
    assert "DD_DEPTH_MB" not in os.environ
    os.environ["DD_DEPTH_MB"] = "1"
    try:
        got = eng.exact_cover(fixture_paths, many, k, 64, clip=3, ntok=NTOK)
    finally:
        del os.environ["DD_DEPTH_MB"]
    found = eng.last_cover_found
    # a sample's share of the budget: its counters and its rows
    rows = sum(-(-t // 64) for t in NTOK)
    per = (1 << 20) // (found * 4 + rows * 24)
    assert per >= 1 and -(-70 // per) >= 5, (found, per)
    assert all(a.shape == (70, -(-t // 64), 6) for a, t in zip(got, NTOK))
    for j in range(7):
        one = eng.exact_cover(fixture_paths, [sample_paths[j]], k, 64, clip=3, ntok=NTOK)
        assert eng.last_cover_found == found
        for g in range(N):
            for row in range(j, 70, 7):
                assert got[g][row].tobytes() == one[g][0].tobytes(), (g, row)
    same([a[:7] for a in got], want(k, True, 64, 3), "the first seven")


# ---- 6. two calls, the device form --------------------------------------------------------------------------------------------
def test_two_calls_and_the_device_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = gs.samples()[2][2]
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    for k in (21, 62):
        for window, targets in ((192, None), (64, [3, 1])):
            a = eng.exact_cover(fixture_paths, sample_paths, k, window, targets=targets, clip=7)
            found = eng.last_cover_found
            b = eng.exact_cover(fixture_paths, sample_paths, k, window, targets=targets, clip=7)
            dev = eng.exact_cover_device(ptrs, sizes, N, k, window, NTOK, targets=targets, clip=7)
            assert found == eng.last_cover_found and len(a) == len(b) == len(dev) == (N if targets is None else 2)
            for x, y, z in zip(a, b, dev):
                assert x.tobytes() == y.tobytes() == z.tobytes() and x.shape == z.shape, (k, window)
            w = want(k, True, window, 7)
            same(a, w if targets is None else [w[g] for g in targets], (k, window))
            assert any(x[..., 1].any() for x in a)


# ---- 7. the argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], sample_paths[:2]

    def call(paths=paths, smp=smp, k=11, targets=(0, 2), nt=None, window=64, clip=3, off=None, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        tg = np.array(list(targets) or [0], dtype=np.int32)
        nt = len(targets) if nt is None else nt
        if off is None:
            w = window if window >= 64 else 64
            off = np.cumsum([0] + [-(-NTOK[t] // w) if 0 <= t < 3 else 1 for t in targets] + [0] * max(nt - len(targets), 0))
        off = np.array(off, dtype=np.uint64)
        counts = np.full((max(ns, 1), max(int(off[-1]), 1), 6), 77, dtype=np.uint32)
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_cover(eng._ctx, None if "paths" in null else pa, n, None if "samples" in null else sa, ns, k,
                                None if "target" in null else tg.ctypes.data, nt, window, clip, None if "off" in null else off.ctypes.data,
                                None if "counts" in null else counts.ctypes.data, None if "found" in null else ctypes.byref(found))
        return rc, counts, found.value, lib.dd_last_error().decode()

    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    ends = [cpur.ends_of(fa, 11, True) for fa in cpur.genomes()[:3]]
    depths = [depth_ref.depths(gs.samples()[j][2], 11, True, masks) for j in range(2)]
    want2 = [[row for g in (0, 2) for row in cover_ref.rows(ends[g], g, NTOK[g], d, masks, 64, 3)] for d in depths]

    def usable():
        rc, counts, found, _ = call()
        assert rc == 0 and found == len(masks) and counts.tolist() == want2
    usable()
    n0, n2 = -(-NTOK[0] // 64), -(-NTOK[2] // 64)
    for kw, text in ((dict(paths=[]), "n=0 outside 1..64"), (dict(paths=paths[:1] * 65), "n=65 outside 1..64"),
                     (dict(smp=[]), "ns=0 outside 1..1024"), (dict(smp=smp[:1] * 1025), "ns=1025 outside 1..1024"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(targets=(), nt=0), "nt=0 outside 1..3"), (dict(targets=(0, 1, 2, 0), nt=4), "nt=4 outside 1..3"),
                     (dict(targets=(0, -1)), "target 1: input -1 outside 0..2"), (dict(targets=(3, 0)), "target 0: input 3 outside 0..2"),
                     (dict(targets=(2, 0, 2)), "target 2: input 2 is target 0 already"),
                     (dict(window=0), "window=0: a multiple of 64 in 64..4194304"), (dict(window=63), "window=63: a multiple of 64"),
                     (dict(window=96), "window=96: a multiple of 64"), (dict(window=(1 << 22) + 64), "window=4194368: a multiple of 64"),
                     (dict(clip=0), "clip=0 outside 1..1023"), (dict(clip=1024), "clip=1024 outside 1..1023"),
                     (dict(off=[0, n0, n0 + n2 - 1]), f"target 1: off[2] - off[1] = {n2 - 1} rows, {n2} expected (input 2 holds {NTOK[2]} tokens, 64 to a window)"),
                     (dict(off=[0, n0 + 1, n0 + 1 + n2]), f"target 0: off[1] - off[0] = {n0 + 1} rows, {n0} expected (input 0 holds {NTOK[0]} tokens"),
                     (dict(off=[5, 4, 4 + n2]), "off[] must ascend"),
                     (dict(null=("paths",)), "null argument"), (dict(null=("samples",)), "null argument"), (dict(null=("target",)), "null argument"),
                     (dict(null=("off",)), "null argument"), (dict(null=("counts",)), "null argument"), (dict(null=("found",)), "null argument")):
        rc, counts, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert (counts == 77).all() and found == 77, kw                    # the outputs are untouched
        usable()
    # off[0] > 0: the rows in front of a sample's share are not the call's
    rc, counts, found, _ = call(off=[2, 2 + n0, 2 + n0 + n2])
    assert rc == 0 and (counts[:, :2] == 77).all() and counts[:, 2:].tolist() == want2
    be = HipExactBackend()
    try:
        assert be.cover_counts([[f"leaf{i}.k11"] for i in range(65)], 11, smp, 64, [0], 255) is None
    finally:
        be.close()


# ---- 8. degenerate inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    paths, smp, fas = gs.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    ntok = [cpur.index_of(fa)[2] for fa in fas[:3]]
    nwin = 1 if kind == "no record" else 0
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gs.BARREN_KS:
            got = eng.exact_cover(paths, smp, k, 64)
            assert len(got) == 3 and all(a.shape == (3, nwin, 6) and not a.any() for a in got) and eng.last_cover_found == 0, (kind, canonical, k)
    dev = eng.exact_cover_device(ptrs, sizes, 3, gs.BARREN_KS[-1], 4096, ntok, targets=[2, 0])
    assert eng.last_cover_found == 0 and len(dev) == 2 and all(a.shape == (3, nwin, 6) and not a.any() for a in dev)


def test_a_target_without_a_token(engine_factory, fixture_paths, sample_paths):
    """g6 is an empty file: as the only target it owns no row, and the call still counts the universe; g5 (41 tokens, shorter
    than k) owns one all-zero row"""
    eng = engine_factory()
    got = eng.exact_cover(fixture_paths, sample_paths, 33, 64, targets=[6])
    assert len(got) == 1 and got[0].shape == (7, 0, 6) and eng.last_cover_found == len(cpur.reference(33, True)[1])
    got = eng.exact_cover(fixture_paths, sample_paths, 61, 64, targets=[6, 5, 1])
    assert got[0].shape == (7, 0, 6) and got[1].shape == (7, 1, 6) and not got[1].any()
    assert got[2].tolist() == want(61, True, 64, 255)[1].tolist()


# ---- 9. the command -----------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen --cover 64 --cover-clip 3 --cover-min 50` on a real `--exact` tree (HipExactBackend), as a process of its own:
    the three CSVs equal the tables cover_ref computes from the files' text."""
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
    reads.write_bytes(gs.samples()[2][1])
    order = [s["leaf"], s["rel"], str(reads), s["far"], s["none"]]
    out = str(tmp_path / "o")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-g", gfile, "-k", "12", "-k", "33", "--cover", "64",
                        "--cover-clip", "3", "--cover-min", "50", "-o", out, *order], env=env, cwd=gs.ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, gs.samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = read_cover(out)
    want_tables = cover_ref.tables(universe, texts, [12, 33], 64, clip=3, min_percent=50)
    assert sorted(got) == ["cover", "cover_regions", "cover_summary"]
    for name in want_tables:
        assert got[name] == want_tables[name], name
    assert len(got["cover_summary"]) == 5 * 2 * 5
    assert {"present", "absent"} <= {r[3] for r in got["cover_regions"]}
