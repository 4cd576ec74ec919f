"""dd_exact_reads on the MI355X: every array -- counts, calls, sets, tally -- compared with == against reads_ref (k-mer ends
and masks from Python dictionaries, rows by bisect, the vote by the header's rules) over the fixture of test_core_regions and
the seven samples of test_gpu_screen with records for rows; reads of several genomes; empty and one-token rows, borders at
wave and workgroup edges; borders that are windows against dd_exact_paint, byte for byte; the tally against the calls;
passes and determinism; 70 samples in one call and the device form; a universe without a record; the argument rules; and
`screen --reads --reads-calls` end to end on a real `--exact` tree."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pyref
import reads_ref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_gpu_paint as gpup
import test_gpu_screen as gpus
import test_reads as cpurd
import test_screen as cpus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = gpus.KS
KS_NOCANON = gpus.KS_NOCANON
DD_EINVAL = -1
N = 7
MIN_HITS = (1, 100)
S2_UNIQUE, S2_AMBIGUOUS = 377, 23      # S2's 400 reads at k = 33 and 61, min_hits = 1


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("reads_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads_samples")
    paths = []
    for name, raw, _ in gpus.samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


def records_of(j):
    return cpur.index_of(gpus.samples()[j][2])[1]


@functools.lru_cache(maxsize=None)
def want(j, k, canonical, min_hits):
    """(counts, calls, sets, classes, tally) of sample j with its records for rows, from reads_ref: a computation of its own,
    never changed"""
    _, masks = cpur.reference(k, canonical)
    return reads_ref.answer(gpus.samples()[j][2], k, canonical, masks, N, records_of(j), min_hits, ends=gpup.sample_ends(j, k, canonical))


def same(got, wanted, n, what):
    """one sample's (calls, sets, counts) of the engine against (counts, calls, sets, ..) of the reference"""
    calls, sets, counts = got
    rows = len(wanted[0])
    assert calls.dtype == np.uint32 and calls.shape == (rows, 6) and sets.dtype == np.uint64 and sets.shape == (rows, 2), what
    assert counts.dtype == np.uint32 and counts.shape == (rows, n + 2), what
    assert counts.tolist() == wanted[0], what
    assert calls.tolist() == wanted[1], what
    assert sets.tolist() == wanted[2], what


# ---- 1. every array against the reference -------------------------------------------------------------------------------------
def test_the_reference_holds_every_class():
    """(no GPU work: the fixture does what it is for)"""
    nrec = [len(records_of(j)) for j in range(7)]
    assert nrec == [1, 1, 400, 0, 1, 1, 1] and gpup.ntoks()[1] == 20_001        # S1: one row of 313 segments
    for k in (33, 61):
        _, calls, sets, classes, tally = want(2, k, True, 1)
        assert sum(tally[:N]) == S2_UNIQUE and tally[N:] == [S2_AMBIGUOUS, 0, 0], (k, tally)
    assert want(2, 33, True, 100)[4] == want(2, 33, True, 1)[4]                  # 150 - 33 + 1 = 118 positions: the calls stand
    assert want(2, 61, True, 100)[4] == [0] * N + [0, 400, 0]                    # 150 - 61 + 1 = 90 < 100: nothing is called
    for canonical, ks in ((True, KS), (False, KS_NOCANON)):
        for k in ks:
            _, calls, sets, classes, tally = want(0, k, canonical, 1)            # S0 is g0 = g4 byte for byte
            assert classes == [N] and sets[0] == [0b10001, 0b10001] and calls[0][2] == 0 and calls[0][4] == 4, (k, canonical)
            assert calls[0][0] == calls[0][1] == calls[0][3] == calls[0][5] == 6000 - k + 1
            if k >= 16:
                assert want(5, k, canonical, 1)[3] == [N + 1], k                 # S5: unrelated text
            assert want(4, k, canonical, 1)[3] == ([N + 2] if k >= 41 else want(4, k, canonical, 1)[3]), k
            assert want(3, k, canonical, 1)[4] == [0] * (N + 3)


@pytest.mark.parametrize("canonical,k", [(True, k) for k in KS] + [(False, k) for k in KS_NOCANON])
def test_every_array_equals_the_reference(engine_factory, fixture_paths, sample_paths, canonical, k):
    """One call over S0..S6 with records for rows: S1 is one row of 313 segments (the wave-uniform path, five waves, two
    workgroups), S2 400 reads of 150 bases (a border inside every wave, 2-3 segments to a row), S3 has no row, S4 is 40 bases,
    S6 has BREAKs (N, R) that are no borders."""
    eng = engine_factory(canonical=canonical)
    for min_hits in MIN_HITS:
        per, tally = eng.exact_reads(fixture_paths, sample_paths, k, min_hits=min_hits, counts=True)
        assert eng.last_sketch_stats()[2] == 1 and eng.last_reads_found == len(cpur.reference(k, canonical)[1])
        assert len(per) == 7 and tally.dtype == np.uint64 and tally.shape == (7, N + 3)
        for j in range(7):
            w = want(j, k, canonical, min_hits)
            same(per[j], w, N, (k, canonical, min_hits, j))
            assert tally[j].tolist() == w[4], (k, canonical, min_hits, j)
        assert per[3][0].shape == (0, 6) and not tally[3].any()
        assert tally[4].tolist() == [0] * (N + 2) + [1] or k < 41


# ---- 2. several targets ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_reads():
    """-> (FASTA bytes, FASTQ bytes, text): 48 reads of 150 bases drawn in turn from g0..g3 of the fixture"""
    rng = np.random.default_rng(20261020)
    texts = [b"".join(pyref.records(cpur.genomes()[g])).decode().upper() for g in range(4)]
    reads = []
    for j in range(48):
        t = texts[j % 4]
        p = int(rng.integers(0, len(t) - 150))
        reads.append(t[p:p + 150])
    fa = "".join(f">m{j} g{j % 4}\n{r}\n" for j, r in enumerate(reads)).encode()
    fq = "".join(f"@m{j} g{j % 4}\n{r}\n+\n{'F' * 150}\n" for j, r in enumerate(reads)).encode()
    return fa, fq, fa


@pytest.mark.parametrize("k", [21, 33])
def test_reads_of_several_genomes(engine_factory, fixture_paths, tmp_path, k):
    eng = engine_factory()
    fa, fq, text = mixed_reads()
    (tmp_path / "m.fa").write_bytes(fa)
    (tmp_path / "m.fq").write_bytes(fq)
    _, masks = cpur.reference(k, True)
    borders = cpur.index_of(text)[1]
    w = reads_ref.answer(text, k, True, masks, N, borders, 1)
    assert sum(1 for c in w[4][:N] if c) >= 3 and w[4][N] >= 1, w[4]             # the reference alone: three targets, an ambiguous row
    per, tally = eng.exact_reads(fixture_paths, [str(tmp_path / "m.fa"), str(tmp_path / "m.fq")], k, counts=True)
    for j in range(2):
        same(per[j], w, N, (k, j))
        assert tally[j].tolist() == w[4]


# ---- 3. short and empty rows, borders at wave and workgroup edges -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted(k):
    """records of 0, 0, 1, k - 1, k, k + 1, 63, 64 and 65 bases, forty of 5..30 (several borders in one thread's segment, runs
    of one-token rows), then lengths that put borders at the tokens 4095, 4096, 4097 and 16 383, 16 384"""
    rng = np.random.default_rng(4096 + k)
    pool = "".join(b"".join(pyref.records(cpur.genomes()[g])).decode().upper() for g in (1, 2, 3, 0))
    lens = [0, 0, 1, k - 1, k, k + 1, 63, 64, 65] + [int(v) for v in rng.integers(5, 31, 40)]
    lens[12:12] = [0, 0, 0]                                   # a run of one-token rows among the short ones
    at = sum(1 + n for n in lens)                             # the tokens so far; the next record's first base is token at + 1
    lens.append(4095 - (at + 1) - 1)                          # ... and ends at 4093: the next BREAK is 4094, the next border 4095
    lens += [0, 0, 16_383 - 4097 - 1, 0, 500]
    recs, p = [], 0
    for n in lens:
        recs.append(pool[p:p + n])
        p += n
    assert p <= len(pool)
    fa = "".join(f">c{j}\n{r}\n" for j, r in enumerate(recs)).encode()
    return fa


@pytest.mark.parametrize("k", [11, 33])
def test_short_and_empty_rows(engine_factory, fixture_paths, tmp_path, k):
    eng = engine_factory()
    fa = crafted(k)
    (tmp_path / "c.fa").write_bytes(fa)
    lens, borders, ntok = cpur.index_of(fa)
    assert {4095, 4096, 4097, 16_383, 16_384} <= set(borders) and ntok == 16_384 + 500
    assert lens[:9] == [0, 0, 1, k - 1, k, k + 1, 63, 64, 65]
    assert max(sum(1 for b in borders if 64 * s <= b < 64 * s + 64) for s in range(ntok // 64)) >= 4
    _, masks = cpur.reference(k, True)
    for min_hits in (1, 20):
        w = reads_ref.answer(fa, k, True, masks, N, borders, min_hits)
        assert w[4][N + 2] >= 9 and sum(w[4][:N + 1]) >= 5, w[4]                 # rows without a k-mer, and called ones
        per, tally = eng.exact_reads(fixture_paths, [str(tmp_path / "c.fa")], k, min_hits=min_hits, counts=True)
        same(per[0], w, N, (k, min_hits))
        assert tally[0].tolist() == w[4]
    assert [r[0] for r in w[0][:6]] == [0, 0, 0, 0, 1, 2]


# ---- 4. borders that are windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_window_borders_equal_paint_on_s1(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    ntok = gpup.ntoks()[1]
    for window in (64, 4096):
        paint = eng.exact_paint(fixture_paths, [sample_paths[1]], k, window, ntok=[ntok])[0]
        per, tally = eng.exact_reads(fixture_paths, [sample_paths[1]], k, rows=[np.arange(0, ntok, window)], counts=True)
        assert per[0][2].shape == paint.shape and per[0][2].tobytes() == paint.tobytes(), (k, window)
        assert paint.tolist() == gpup.want(1, k, True, window) and int(tally.sum()) == len(paint)


@pytest.mark.parametrize("k", [11, 33])
def test_window_borders_equal_paint_on_the_wide_universe(engine_factory, tmp_path, k):
    """all seven planes, bit 63, and a row with 64 in all 66 columns"""
    eng = engine_factory()
    paths = greedy.write(tmp_path, gpup.wide_universe())
    for window in (64, 4096):
        rows, found = gpup.wide_want(k, window)
        paint = eng.exact_paint(paths, [paths[63]], k, window)[0]
        per, tally = eng.exact_reads(paths, [paths[63]], k, rows=[np.arange(0, 4001, window)], counts=True)
        calls, sets, counts = per[0]
        assert eng.last_reads_found == found and counts.tobytes() == paint.tobytes() and counts.tolist() == rows, (k, window)
        votes = [reads_ref.vote(r, 64, 1) for r in rows]
        assert calls.tolist() == [v[0] for v in votes] and sets.tolist() == [v[1] for v in votes]
        assert tally[0].tolist() == [sum(1 for v in votes if v[2] == c) for c in range(67)]
        if window == 64:
            full = [i for i, r in enumerate(counts.tolist()) if r == [64] * 66]
            assert full and all(sets[i].tolist() == [2 ** 64 - 1, 2 ** 64 - 1] for i in full)
            assert (sets[:, 0] >> np.uint64(63)).any()


# ---- 5. the tally ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_hits", [(21, 1), (61, 80)])
def test_tally_is_the_sum_of_the_calls(engine_factory, fixture_paths, sample_paths, k, min_hits):
    from dandd_amd.engine import read_classes
    eng = engine_factory()
    per, tally = eng.exact_reads(fixture_paths, sample_paths, k, min_hits=min_hits)
    for j, (calls, sets, counts) in enumerate(per):
        assert counts is None
        classes, mine = read_classes(calls, sets, min_hits, N)
        assert mine.tolist() == tally[j].tolist() and classes.tolist() == want(j, k, True, min_hits)[3], (k, j)
        assert int(tally[j].sum()) == len(records_of(j))
    only, tally2 = eng.exact_reads(fixture_paths, sample_paths, k, min_hits=min_hits, calls=False)
    assert all(p == (None, None, None) for p in only) and tally2.tobytes() == tally.tobytes() and tally.any()


# ---- 6. passes and determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 62])
def test_multi_pass_gives_identical_bytes(engine_factory, tmp_path, k):
    """test_gpu_paint's 17 x 19 kbp universe with a 1 MiB sort budget; rows of 150 tokens"""
    eng = engine_factory()
    family = greedy.related(18, 19_000, 17)
    paths = greedy.write(tmp_path, family[:17])
    other = greedy.write(tmp_path, family[17:], tag="x")
    smp = [paths[5], other[0]]
    rows = [np.arange(0, 19_001, 150)] * 2
    assert "DD_EXACT_MB" not in os.environ

    def call():
        per, tally = eng.exact_reads(paths, smp, k, min_hits=5, rows=rows, counts=True)
        return b"".join(a.tobytes() for p in per for a in p) + tally.tobytes(), per, tally
    one, per, tally = call()
    found = eng.last_reads_found
    assert eng.last_sketch_stats()[2] == 1
    again = call()[0]
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = call()[0]
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_reads_found > 65_536
    assert one == again == many
    # a genome of the universe: every position is there, and in itself
    assert per[0][2][:, 0].sum() == 19_000 - k + 1 and (per[0][2][:, 0] == per[0][2][:, 2 + 5]).all()
    assert (per[0][1][:, 1] >> np.uint64(5) & np.uint64(1)).all() and int(tally[0].sum()) == len(rows[0])


# ---- 7. many samples, one call; the device form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 61])
def test_seventy_samples_in_one_call(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    index = [(None, None, records_of(j), None) for j in range(7)]
    many, tally = eng.exact_reads(fixture_paths, [sample_paths[j % 7] for j in range(70)], k, index=[index[j % 7] for j in range(70)], counts=True)
    found = eng.last_reads_found
    assert len(many) == 70 and tally.shape == (70, N + 3)
    for j in range(7):
        one, t1 = eng.exact_reads(fixture_paths, [sample_paths[j]], k, counts=True)
        assert eng.last_reads_found == found
        same(one[0], want(j, k, True, 1), N, (k, j))
        for row in range(j, 70, 7):
            assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(many[row], one[0])), (k, row)
            assert tally[row].tobytes() == t1[0].tobytes()


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = gpus.samples()[2][2]
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    rows = [records_of(j) for j in range(7)]
    for k, min_hits in ((21, 1), (62, 50)):
        dev, dt = eng.exact_reads_device(ptrs, sizes, N, k, rows, min_hits=min_hits, counts=True)
        path, pt = eng.exact_reads(fixture_paths, sample_paths, k, min_hits=min_hits, counts=True)
        assert len(dev) == len(path) == 7 and path[0][0].any() and dt.tobytes() == pt.tobytes()
        assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for d, p in zip(dev, path) for a, b in zip(d, p)), k


# ---- 8. a universe that leaves the emission nothing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    """test_gpu_screen's barren universes: column 0 is the sample's own, every row with a valid k-mer is unclassified"""
    paths, smp, fas = gpus.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gpus.on_device(torch_cuda, fas)
    texts = [gpus.samples()[j][2] for j in gpus.BARREN_SAMPLES]
    rows = [cpur.index_of(text)[1] for text in texts]
    assert [len(r) for r in rows] == [1, 0, 1]
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gpus.BARREN_KS:
            per, tally = eng.exact_reads(paths, smp, k, counts=True)
            assert eng.last_reads_found == 0 and len(per) == 3
            for text, r, got in zip(texts, rows, per):
                same(got, reads_ref.answer(text, k, canonical, {}, 3, r, 1), 3, (kind, canonical, k))
                assert not got[2][:, 1:].any() and not got[1].any()
            assert per[0][2][0, 0] == 6000 - k + 1
            assert tally.tolist() == [[0, 0, 0, 0, 1, 0], [0] * 6, [0, 0, 0, 0, 1, 0] if k <= 40 else [0, 0, 0, 0, 0, 1]]
    dev, dt = eng.exact_reads_device(ptrs, sizes, 3, k, rows, counts=True)
    assert eng.last_reads_found == 0 and dt.tobytes() == tally.tobytes()
    assert all(a.tobytes() == b.tobytes() for d, p in zip(dev, per) for a, b in zip(d, p))


# ---- 9. the argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], [sample_paths[2], sample_paths[3], sample_paths[1]]
    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    texts = [gpus.samples()[j][2] for j in (2, 3, 1)]
    borders = [cpur.index_of(t)[1] for t in texts]
    nt = [cpur.index_of(t)[2] for t in texts]
    assert [len(b) for b in borders] == [400, 0, 1] and nt == [60_400, 0, 20_001]
    want3 = [reads_ref.answer(t, 11, True, masks, 3, b, 1) for t, b in zip(texts, borders)]

    def call(paths=paths, smp=smp, k=11, borders=borders, min_hits=1, off=None, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        if off is None:
            off = np.zeros(max(ns, 0) + 1, dtype=np.uint64)
            off[1:1 + len(borders)] = np.cumsum([len(b) for b in borders[:ns]], dtype=np.uint64) if ns else []
        off = np.asarray(off, dtype=np.uint64)
        start = np.array([v for b in borders for v in b] + [0], dtype=np.uint64)
        rows, nn = max(int(off.max()), 1) + 1, min(n, 64)
        out = dict(calls=np.full((rows, 6), 77, dtype=np.uint32), sets=np.full((rows, 2), 77, dtype=np.uint64),
                   counts=np.full((rows, nn + 2), 77, dtype=np.uint32), tally=np.full((max(ns, 1) + 1, nn + 3), 77, dtype=np.uint64))
        found = ctypes.c_uint64(77)
        ptr = lambda name, a: None if name in null else a.ctypes.data
        rc = lib.dd_exact_reads(eng._ctx, pa, n, sa, ns, k, ptr("off", off), ptr("start", start), min_hits, ptr("calls", out["calls"]),
                                ptr("sets", out["sets"]), ptr("counts", out["counts"]), ptr("tally", out["tally"]),
                                None if "found" in null else ctypes.byref(found))
        return rc, out, found.value, lib.dd_last_error().decode()

    def untouched(out, found):
        return all((a == 77).all() for a in out.values()) and found == 77

    def usable(null=()):
        rc, out, found, err = call(null=null)
        assert rc == 0 and found == len(masks), err
        for name, col in (("counts", 0), ("calls", 1), ("sets", 2)):
            if name in null:
                assert (out[name] == 77).all()
            else:
                assert out[name][:-1].tolist() == want3[0][col] + want3[2][col] and (out[name][-1] == 77).all(), name
        assert out["tally"][:-1].tolist() == [w[4] for w in want3] and (out["tally"][-1] == 77).all()
    usable()
    usable(null=("calls",))
    usable(null=("calls", "sets", "counts"))
    bad = lambda j, r, v: [b if i != j else list(b[:r]) + [v] + list(b[r + 1:]) for i, b in enumerate(borders)]
    cases = [(dict(min_hits=0), "min_hits=0"),
             (dict(borders=bad(0, 7, borders[0][6])), "sample 0, row 7"), (dict(borders=bad(0, 7, borders[0][6] - 1)), "sample 0, row 7"),
             (dict(borders=bad(0, 399, nt[0] + 1)), "sample 0, row 399"), (dict(borders=bad(2, 0, nt[2] + 1)), "sample 2, row 0"),
             (dict(off=[0, 400, 399, 401]), "off[] must ascend"), (dict(off=[5, 4, 4, 4]), "off[] must ascend"),
             (dict(smp=[], borders=[]), "ns=0 outside 1..1024"), (dict(smp=smp[1:2] * 1025, borders=[[]] * 1025), "ns=1025 outside 1..1024"),
             (dict(paths=paths[:1] * 65), "n=65 outside 1..64"), (dict(paths=[]), "n=0 outside 1..64"),
             (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
             (dict(null=("tally",)), "null argument"), (dict(null=("off",)), "null argument"), (dict(null=("start",)), "null argument"),
             (dict(null=("found",)), "null argument")]
    for kw, text in cases:
        rc, out, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert untouched(out, found), kw                                     # the outputs are untouched
    usable()
    assert f"{nt[0]} tokens" in call(borders=bad(0, 399, nt[0] + 1))[3]
    # a border AT the sample's end is legal (an empty last row), and so is a first border of 0
    rc, out, found, err = call(smp=smp[2:], borders=[[0, nt[2]]])
    edge = reads_ref.answer(texts[2], 11, True, masks, 3, [0, nt[2]], 1)
    assert rc == 0 and out["calls"][1].tolist() == [0, 0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0] and edge[4][5] == 1 and sum(edge[4]) == 2, err
    assert out["tally"][0].tolist() == edge[4] and out["calls"][:2].tolist() == edge[1] and out["sets"][:2].tolist() == edge[2]
    assert out["counts"][:2].tolist() == edge[0] and edge[0][0] == want3[2][0][0]
    # no row asked for: start may be null
    rc, out, found, err = call(smp=smp[1:2] * 2, borders=[[], []], null=("start", "calls", "sets", "counts"))
    assert rc == 0 and found == len(masks) and not out["tally"][:2].any(), err
    be = HipExactBackend()
    try:
        assert be.read_calls([[f"leaf{i}.k11"] for i in range(65)], 11, smp, 1, True) is None
    finally:
        be.close()


# ---- 10. the command -----------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen --reads --reads-calls` on a real `--exact` tree (HipExactBackend), as processes of their own: both CSVs equal
    the tables reads_ref computes from the files' text, the screen files are what they are without --reads."""
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
    order = [s["leaf"], s["rel"], cpurd._reads_sample(tmp_path, data), str(reads), s["far"], s["none"]]
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    outs = {}
    for name, extra in (("plain", []), ("reads", ["--reads", "--reads-calls", "--reads-min-hits", "3"])):
        outs[name] = str(tmp_path / name)
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-k", "12", "-k", "33", "-o", outs[name], *extra,
                            *order], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, gpus.samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = cpurd.read_reads(outs["reads"])
    want = reads_ref.tables(universe, texts, [12, 33], min_hits=3)
    assert sorted(got) == ["reads", "reads_summary"]
    for name in want:
        assert got[name] == want[name], name
    assert not cpurd.read_reads(outs["plain"]) and len(got["reads"]) == 2 * (2 + 2 + 21 + 400 + 1)
    before, after = cpus.read_csvs(outs["plain"]), cpus.read_csvs(outs["reads"])
    assert sorted(before) == ["screen", "screen_summary"] and before == after
