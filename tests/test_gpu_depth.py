"""dd_exact_depth on the MI355X: every cell of hist / total compared with == against depth_ref (a collections.Counter over
pyref.kmers, restricted to the universe's masks) over test_gpu_screen's universe, samples and queries, in both strand modes
and at 8 and 256 bins; the identities with dd_exact_screen and dd_exact_paint; a counter past 16 bits and the overflow sum;
more rows than one LDS tile; samples taken in rounds; records accumulated over passes; two calls byte for byte; the device
form; the argument rules; degenerate inputs; and `screen --depth` end to end on a real `--exact` tree."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_ref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_gpu_screen as gs
import test_screen as cpus
from test_depth import read_depth

pytestmark = pytest.mark.gpu

N = gs.N
DD_EINVAL = -1
BINS = (8, 256)


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("depth_universe"))


@pytest.fixture(scope="module")
def sample_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_samples")
    paths = []
    for name, raw, _ in gs.samples():
        (d / name).write_bytes(raw)
        paths.append(str(d / name))
    return paths


def split(qs):
    return [a for a, _ in qs], [b for _, b in qs]


@functools.lru_cache(maxsize=None)
def want(k, canonical, bins, qs=None):
    """-> (hist [7][N+nq][bins], total [7][N+nq], found) of S0..S6 from depth_ref: a computation of its own, never changed"""
    masks = cpur.reference(k, canonical)[1]
    got = [depth_ref.answer(text, k, canonical, masks, N, list(qs or gs.queries()), bins) for _, _, text in gs.samples()]
    return np.array([h for h, _ in got], dtype=np.uint64), np.array([t for _, t in got], dtype=np.uint64), len(masks)


# ---- 1. every cell against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in gs.KS] + [(False, k) for k in gs.KS_NOCANON])
def test_every_cell_equals_the_reference(engine_factory, fixture_paths, sample_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    qs = gs.queries()
    for bins in BINS:
        hist, total = eng.exact_depth(fixture_paths, sample_paths, k, *split(qs), bins=bins)
        assert eng.last_sketch_stats()[2] == 1
        w_hist, w_total, w_found = want(k, canonical, bins)
        assert hist.dtype == np.uint64 and total.dtype == np.uint64
        assert hist.shape == (7, N + len(qs), bins) and total.shape == (7, N + len(qs))
        assert eng.last_depth_found == w_found
        for s in range(7):
            assert hist[s].tolist() == w_hist[s].tolist(), (k, canonical, bins, s)
        assert total.tolist() == w_total.tolist(), (k, canonical, bins)
    # the fixture does what it is for (the last `hist` has 256 bins, w8 has 8): the pan-genome's row, N
    w8 = want(k, canonical, 8)[0]
    pan = hist[:, N, :]
    assert w8[2, N, 1:].all()                                            # S2: every bin 1..7, the clipped one included
    assert pan[2, 8:].any() and pan[1, 2:5].all()                        # ... its depths go on behind 7; S1 spreads over 2..4 at least
    if k >= 21:
        assert pan[0, 1] > 5000 and not pan[0, 2:].any()                 # S0: all at depth 1, the one-bin path of the tally
        assert pan[1, 1:5].all() and not pan[1, 5:].any()                # S1: 1..4
    deep = np.flatnonzero(pan[6, 1:]) + 1                                # S6: one or two records, many adds on one counter
    assert 1 <= pan[6, 1:].sum() <= 2 and len(deep) == 1 and 7 <= deep[0] <= 120 and (canonical is False or deep[0] >= 14)
    assert not pan[3, 1:].any() and not pan[4, 1:].any() and pan[5, 1:].sum() <= 13 and not total[3].any()
    assert not hist[:, -1, :].any() and not total[:, -1].any()            # the (all & none) pair matches nothing


# ---- 2. identities with entry points that exist ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_identities_with_screen_and_paint(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    qs = gs.queries()
    al, no = split(qs)
    hist, total = eng.exact_depth(fixture_paths, sample_paths, k, al, no, bins=8)
    shared, match = eng.exact_screen(fixture_paths, sample_paths, k, al, no)
    assert eng.last_depth_found == eng.last_screen_found
    ns = len(sample_paths)
    for s in range(ns):
        assert hist[s].sum(-1)[:N].tolist() == shared[ns].tolist() and hist[s].sum(-1)[N:].tolist() == match[ns].tolist(), s
        assert hist[s, :, 1:].sum(-1)[:N].tolist() == shared[s].tolist() and hist[s, :, 1:].sum(-1)[N:].tolist() == match[s].tolist(), s
    painted = eng.exact_paint(fixture_paths, sample_paths, k, 64)
    for s, counts in enumerate(painted):
        counts = counts.astype(np.uint64)
        assert total[s, :N].tolist() == counts[:, 2:].sum(0).tolist(), s
        assert int(total[s, N]) == int(counts[:, 1].sum()), s              # the (0, 0) row: every position in the pan-genome
    assert total[2, N] > 30_000 and total[0, N] > 5000


# ---- 3. a counter past 16 bits, and the overflow sum -----------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, 21), (True, 33), (False, 64)])
def test_a_counter_past_sixteen_bits(engine_factory, fixture_paths, sample_paths, tmp_path, canonical, k):
    eng = engine_factory(canonical=canonical)
    text = (">poly\n" + "A" * 70_000 + "\n").encode()                     # 1094 segments, every k-mer the same record
    path = tmp_path / "poly.fa"
    path.write_bytes(text)
    qs = gs.queries()
    masks = cpur.reference(k, canonical)[1]
    assert masks[0] == 1 << 3                                            # A^k is a record of the universe: g3's A^70 run (and, canonical, its T^70)
    w_hist, w_total = depth_ref.answer(text, k, canonical, masks, N, qs, 8)
    assert w_total[3] == w_total[N] == 70_001 - k > 1 << 16 and w_hist[3][7] == 1 and w_hist[3][0] == sum(w_hist[3]) - 1
    hist, total = eng.exact_depth(fixture_paths, [str(path), sample_paths[6]], k, *split(qs), bins=8)
    assert hist[0].tolist() == w_hist and total[0].tolist() == w_total
    assert hist[1].tolist() == want(k, canonical, 8)[0][6].tolist() and total[1].tolist() == want(k, canonical, 8)[1][6].tolist()


# ---- 4. more rows than one LDS tile ----------------------------------------------------------------------------------------
def many_queries():
    """130 queries: queries() nine times over with a single-genome query behind each, every genome's private pair, pairs of
    neighbours"""
    base, full = gs.queries(), (1 << N) - 1
    qs = []
    for j in range(9):
        qs.extend(base)
        qs.append((1 << (j % N), 0))
    return qs + [(1 << i, full ^ (1 << i)) for i in range(N)] + [(3 << i, 0) for i in range(N - 1)]


def test_row_tiles(engine_factory, fixture_paths, sample_paths):
    eng = engine_factory()
    qs = many_queries()
    assert len(qs) == 130 and len(set(qs)) >= 25
    # (a row of 256 bins is 1 KiB of LDS and more, a workgroup's tile 72 KiB -- kDepthTileBytes --: 137 rows are two tiles)
    assert (N + len(qs)) * 256 * 4 > 72 * 1024
    k = 33
    hist, total = eng.exact_depth(fixture_paths, sample_paths, k, *split(qs), bins=256)
    w_hist, w_total, _ = want(k, True, 256, tuple(qs))
    assert hist.tolist() == w_hist.tolist() and total.tolist() == w_total.tolist()
    h1, t1 = eng.exact_depth(fixture_paths, sample_paths, k, *split(qs[:65]), bins=256)
    h2, t2 = eng.exact_depth(fixture_paths, sample_paths, k, *split(qs[65:]), bins=256)
    assert hist[:, :N + 65].tobytes() == h1.tobytes() and hist[:, N + 65:].tobytes() == h2[:, N:].tobytes()
    assert total[:, :N + 65].tobytes() == t1.tobytes() and total[:, N + 65:].tobytes() == t2[:, N:].tobytes()
    assert hist[:, N + 65:, 1:].any()


# ---- 5. samples taken in rounds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 61])
def test_seventy_samples_in_rounds(engine_factory, fixture_paths, sample_paths, k):
    eng = engine_factory()
    qs = gs.queries()
    al, no = split(qs)
    many = [sample_paths[j % 7] for j in range(70)]
    assert "DD_DEPTH_MB" not in os.environ
    os.environ["DD_DEPTH_MB"] = "1"
    try:
        hist, total = eng.exact_depth(fixture_paths, many, k, al, no, bins=8)
    finally:
        del os.environ["DD_DEPTH_MB"]
    found = eng.last_depth_found
    # a sample's share of the budget: its counters and its histograms; 1 MiB holds 17 of them at the most (k = 61: 13)
    per = (1 << 20) // (found * 4 + (N + len(qs)) * 9 * 8)
    assert 1 <= per <= 17 and -(-70 // per) >= 5, (found, per)
    assert hist.shape == (70, N + len(qs), 8) and total.shape == (70, N + len(qs))
    for j in range(7):
        one_h, one_t = eng.exact_depth(fixture_paths, [sample_paths[j]], k, al, no, bins=8)
        assert eng.last_depth_found == found
        for row in range(j, 70, 7):
            assert hist[row].tobytes() == one_h[0].tobytes() and total[row].tobytes() == one_t[0].tobytes(), (k, row)
    w_hist, w_total, _ = want(k, True, 8)
    assert hist[:7].tolist() == w_hist.tolist() and total[63:].tolist() == w_total.tolist()


# ---- 6. records accumulated over passes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 62])
def test_multi_pass_gives_identical_bytes(engine_factory, tmp_path, k):
    """test_gpu_screen's 17 x 19 kbp universe with a 1 MiB sort budget: at least three passes append their records before the
    one ordering the samples are counted against."""
    eng = engine_factory()
    family = greedy.related(18, 19_000, 17)
    paths = greedy.write(tmp_path, family[:17])
    other = greedy.write(tmp_path, family[17:], tag="x")
    full = (1 << 17) - 1
    qs = [(0, 0), (full, 0), (0b111, 0), (0, full ^ 0b111), (1 << 5, full ^ (1 << 5))]
    al, no = split(qs)
    smp = [paths[5], other[0]]
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_depth(paths, smp, k, al, no, bins=16)
    found = eng.last_depth_found
    assert eng.last_sketch_stats()[2] == 1
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = eng.exact_depth(paths, smp, k, al, no, bins=16)
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_depth_found > 65_536
    assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes()
    hist, total = one
    assert hist[0, 5, 0] == 0 and hist[0, 5, 1:].sum() > 0                 # a genome of the universe: all of it is there
    assert hist[0, 17].sum() == found and 0 < hist[1, 17, 1:].sum() < hist[0, 17, 1:].sum()


# ---- 7. two calls, 8. the device form ---------------------------------------------------------------------------------------
def test_two_calls_return_identical_bytes(engine_factory, fixture_paths, sample_paths):
    eng = engine_factory()
    al, no = split(gs.queries())
    a = eng.exact_depth(fixture_paths, sample_paths, 29, al, no, bins=64)
    b = eng.exact_depth(fixture_paths, sample_paths, 29, al, no, bins=64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0][:, :, 1:].any()
    w_hist, w_total, _ = want(29, True, 64)
    assert a[0].tolist() == w_hist.tolist() and a[1].tolist() == w_total.tolist()


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths, sample_paths):
    eng = engine_factory()
    fas = list(cpur.genomes()) + [cpus.text_of(p) for p in sample_paths]  # (the device form takes text: the FASTQ reads as FASTA)
    fas[N + 2] = gs.samples()[2][2]
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    al, no = split(gs.queries())
    for k in (21, 62):
        dev = eng.exact_depth_device(ptrs, sizes, N, k, al, no, bins=16)
        found = eng.last_depth_found
        path = eng.exact_depth(fixture_paths, sample_paths, k, al, no, bins=16)
        assert path[0][:, :, 1:].any() and found == eng.last_depth_found
        assert dev[0].tobytes() == path[0].tobytes() and dev[1].tobytes() == path[1].tobytes(), k


# ---- 9. the argument rules ---------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths, sample_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    paths, smp = fixture_paths[:3], sample_paths[:2]

    def call(paths=paths, smp=smp, k=11, al=(1, 0), no=(0, 6), nq=None, bins=8, null=()):
        n, ns = len(paths), len(smp)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        sa = (ctypes.c_char_p * max(ns, 1))(*[os.fsencode(p) for p in smp])
        nq = len(al) if nq is None else nq
        a, b = np.array(list(al) or [0], dtype=np.uint64), np.array(list(no) or [0], dtype=np.uint64)
        rows = max(n, 1) + max(nq, 1)
        hist = np.full((max(ns, 1), rows, min(max(bins, 1), 512)), 77, dtype=np.uint64)
        total = np.full((max(ns, 1), rows), 77, dtype=np.uint64)
        found = ctypes.c_uint64(77)
        rc = lib.dd_exact_depth(eng._ctx, pa, n, sa, ns, k, None if "all" in null else a.ctypes.data, None if "none" in null else b.ctypes.data,
                                nq, bins, None if "hist" in null else hist.ctypes.data, None if "total" in null else total.ctypes.data,
                                None if "found" in null else ctypes.byref(found))
        return rc, hist, total, found.value, lib.dd_last_error().decode()

    masks = cpuc.masks_of(cpur.genomes()[:3], 11)
    got = [depth_ref.answer(gs.samples()[j][2], 11, True, masks, 3, [(1, 0), (0, 6)], 8) for j in range(2)]
    want3 = ([h for h, _ in got], [t for _, t in got], len(masks))

    def usable():
        rc, hist, total, found, _ = call()
        assert rc == 0 and found == want3[2] and hist.tolist() == want3[0] and total.tolist() == want3[1]
    usable()
    for kw, text in ((dict(paths=[]), "n=0 outside 1..64"), (dict(paths=paths[:1] * 65), "n=65 outside 1..64"),
                     (dict(smp=[]), "ns=0 outside 1..1024"), (dict(smp=smp[:1] * 1025), "ns=1025 outside 1..1024"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(al=(1, 8)), "query 1: a bit outside 0..2"), (dict(no=(0, 1 << 63)), "query 1: a bit outside 0..2"),
                     (dict(al=(1,) * 1025, no=(0,) * 1025), "nq=1025 outside 0..1024"), (dict(nq=-1), "nq=-1 outside 0..1024"),
                     (dict(bins=1), "bins=1 outside 2..256"), (dict(bins=257), "bins=257 outside 2..256"), (dict(bins=0), "bins=0 outside 2..256"),
                     (dict(null=("hist",)), "null argument"), (dict(null=("total",)), "null argument"), (dict(null=("found",)), "null argument"),
                     (dict(null=("all",)), "null argument"), (dict(null=("none",)), "null argument")):
        rc, hist, total, found, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert (hist == 77).all() and (total == 77).all() and found == 77, kw     # the outputs are untouched
        usable()
    # nq == 0: all and none may be null; the genomes' rows alone
    rc, hist, total, found, _ = call(al=(), no=(), nq=0, null=("all", "none"))
    flat = hist.reshape(-1)                                              # (the answer is [2][3][8]; the buffer has room for a fourth row)
    assert rc == 0 and found == want3[2] and flat[:48].reshape(2, 3, 8).tolist() == [h[:3] for h in want3[0]] and (flat[48:] == 77).all()
    assert total.reshape(-1)[:6].reshape(2, 3).tolist() == [t[:3] for t in want3[1]] and (total.reshape(-1)[6:] == 77).all()
    got = eng.exact_depth(paths, smp, 11, bins=8)
    assert got[0].shape == (2, 3, 8) and got[0].tolist() == [h[:3] for h in want3[0]] and got[1].tolist() == [t[:3] for t in want3[1]]
    # two bins, the least: absent | present
    two = eng.exact_depth(paths, smp, 11, [1, 0], [0, 6], bins=2)
    assert two[0][:, :, 0].tolist() == [[r[0] for r in h] for h in want3[0]] and two[0][:, :, 1].tolist() == [[sum(r[1:]) for r in h] for h in want3[0]]
    assert two[1].tolist() == want3[1]
    be = HipExactBackend()
    try:
        assert be.depth_hists([[f"leaf{i}.k11"] for i in range(65)], 11, smp, [0], [0], 8) is None
    finally:
        be.close()


# ---- 10. degenerate inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_universe_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    paths, smp, fas = gs.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gs.on_device(torch_cuda, fas)
    al, no = [0, 7, 1], [0, 0, 6]
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gs.BARREN_KS:
            hist, total = eng.exact_depth(paths, smp, k, al, no, bins=8)
            assert hist.shape == (3, 6, 8) and total.shape == (3, 6)
            assert not hist.any() and not total.any() and eng.last_depth_found == 0, (kind, canonical, k)
    dev = eng.exact_depth_device(ptrs, sizes, 3, gs.BARREN_KS[-1], al, no, bins=8)
    assert eng.last_depth_found == 0 and not dev[0].any() and not dev[1].any()


def test_an_empty_sample(engine_factory, fixture_paths, sample_paths):
    """S3 (no byte) and S4 (shorter than k) alone, and in front of a sample with hits: everything in bin 0, the sizes of the rows"""
    eng = engine_factory()
    al, no = split(gs.queries())
    w_hist, w_total, _ = want(33, True, 8)
    hist, total = eng.exact_depth(fixture_paths, [sample_paths[3]], 33, al, no, bins=8)
    assert hist[0].tolist() == w_hist[3].tolist() and not total.any() and hist[0, :, 0].any() and not hist[0, :, 1:].any()
    hist, total = eng.exact_depth(fixture_paths, [sample_paths[3], sample_paths[4], sample_paths[2]], 33, al, no, bins=8)
    assert hist.tolist() == w_hist[[3, 4, 2]].tolist() and total.tolist() == w_total[[3, 4, 2]].tolist()


# ---- 11. the command -----------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`screen --depth --depth-hist -g` on a real `--exact` tree (HipExactBackend), as a process of its own: both CSVs equal
    the tables depth_ref computes from the files' text."""
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
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "screen", "-d", pk, "-g", gfile, "-k", "12", "-k", "33", "--depth",
                        "--depth-bins", "8", "--depth-hist", "-o", out, *order], env=env, cwd=gs.ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, gs.samples()[2][2] if p == str(reads) else cpus.text_of(p)) for p in order]
    got = read_depth(out)
    want_tables = depth_ref.tables(universe, texts, [12, 33], groups, bins=8)
    assert sorted(got) == ["depth", "depth_hist"]
    assert got["depth"] == want_tables["depth"] and got["depth_hist"] == want_tables["depth_hist"]
    assert len(got["depth"]) == 5 * 2 * (2 * 5 + 2 + 3 * 3)
