"""dd_exact_locate on the MI355X: every bit of every job's bitmap compared with == against positions built in Python from
pyref.records (test_core_regions.reference), at both key widths and on both sides of each boundary between the two ways a k-mer
carries its genome; the token layout through the (0, 0) job and engine.fasta_index; ties to dd_exact_select and
dd_exact_select_kmers; records accumulated over passes and ordered once; the argument rules; and `core --regions` end to end on
a real `--exact` tree."""
import ctypes
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
import test_gpu_screen as gpus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [11, 28, 29, 32, 33, 60, 61, 64]     # tag in the top byte for 2k <= 56 and 2k - 64 <= 56, in g[] otherwise; 64 | 128-bit keys
KS_NOCANON = [11, 32, 33, 64]
DD_EINVAL = -1


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("regions"))


# ---- G1. every bit against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in KS] + [(False, k) for k in KS_NOCANON])
def test_bitmaps_match_reference(engine_factory, fixture_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    jobs = cpur.group_jobs()
    assert len(jobs) == 3 * 5
    got = eng.exact_locate(fixture_paths, k, jobs)
    assert eng.last_sketch_stats()[2] == 1
    _, masks = cpur.reference(k, canonical)
    assert eng.last_locate_found == sum(1 for m in masks.values() if any(m & a == a and m & b == 0 for a, b, _ in jobs))
    for (a, b, g), words in zip(jobs, got):
        want = cpur.want_bitmap(k, canonical, a, b, g)
        assert words.dtype == np.uint64 and words.shape == want.shape, (k, canonical, hex(a), hex(b), g)
        assert np.array_equal(words, want), (k, canonical, hex(a), hex(b), g)
    # the T run of g3: T^k (canonical: its reverse complement A^k, key 0, which the A run holds too) is a k-mer of g3 alone and is
    # painted at every base of the run from its k-th on -- the all-ones key is also what the slots the single-pass sort never
    # wrote hold
    key = 0 if canonical else (1 << 2 * k) - 1
    ends, _ = cpur.reference(k, canonical)
    at = [t for t, x in ends[3].items() if x == key]
    assert masks[key] == 1 << 3 and len(at) >= (2 if canonical else 1) * (71 - k)
    private = got[jobs.index((0, 127 ^ 8, 3))]
    assert all(int(private[t // 64]) >> (t % 64) & 1 for t in at)


# ---- G2. the layout: where valid k-mers end, from the record index -------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 11, 33])
def test_every_position_is_where_the_index_says(engine_factory, fixture_paths, k):
    from dandd_amd.engine import fasta_index
    eng = engine_factory()
    fas = cpur.genomes()
    n = len(fas)
    index = [fasta_index(p) for p in fixture_paths]
    ntok = [ix[3] for ix in index]
    assert ntok[1] % 64 == 0 and ntok[2] % 64 == 1 and ntok[6] == 0
    got = eng.exact_locate(fixture_paths, k, [(0, 0, g) for g in range(n)], ntok=ntok)
    for g, (fa, (_, seq_len, tok_start, nt), words) in enumerate(zip(fas, index, got)):
        assert len(words) == (nt + 63) // 64
        # a valid k-mer ends at base j of a record iff bases j - k + 1 .. j are all A C G T
        want = []
        for seq, start in zip(pyref.records(fa), tok_start):
            run = 0
            for j, c in enumerate(seq):
                run = run + 1 if c in pyref.CODE else 0
                if run >= k:
                    want.append(int(start) + j)
        assert sum(len(s) for s in pyref.records(fa)) == int(seq_len.sum())
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert np.flatnonzero(bits).tolist() == want, (k, g)
        assert not bits[nt:].any()                                         # bits at or beyond ntok are 0


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [63, 64])
def test_window_warm_up_at_segment_borders(engine_factory, tmp_path, canonical, k):
    """The tightest warm-up of the token walk, in all three kernels that walk (extract, locate, screen): a k-mer that ends on
    the first token of a thread's 64-token segment and needs every other token of the segment in front.  Three records of 197
    bases (tokens 1..197 behind the BREAK at token 0) with one N at token 63, 64 and 65."""
    rng = np.random.default_rng(6364)
    fas = []
    for n_at in (63, 64, 65):
        seq = bytearray(b"ACGT"[c] for c in rng.integers(0, 4, 197))
        seq[n_at - 1] = ord("N")                                           # base j is token j + 1
        fas.append(b">r\n" + bytes(seq) + b"\n")
    paths = greedy.write(tmp_path, fas)
    eng = engine_factory(canonical=canonical)
    want = []
    for fa in fas:
        (seq,) = pyref.records(fa)
        run, ends = 0, []
        for j, c in enumerate(seq):
            run = run + 1 if c in pyref.CODE else 0
            if run >= k:
                ends.append(1 + j)
        want.append(ends)
    # N at token 64: k = 64 leaves one k-mer behind it that ends at token 128, tokens 65..128; k = 63 one in front, at token 63
    assert 128 in want[1] and min(want[1][1:] if k == 63 else want[1]) == 64 + k and (63 in want[1]) == (k == 63)
    got = eng.exact_locate(paths, k, [(0, 0, g) for g in range(3)])
    for g in range(3):
        bits = np.unpackbits(got[g].view(np.uint8), bitorder="little")
        assert len(got[g]) == 4 and np.flatnonzero(bits).tolist() == want[g], (k, canonical, g)
    keys = [set(pyref.kmers(fa, k, canonical)) for fa in fas]
    assert all(len(ks) > 0 for ks in keys)
    for g in range(3):
        assert eng.exact_count([paths[g]], k) == len(keys[g]), (k, canonical, g)
    assert eng.exact_count(paths, k) == len(keys[0] | keys[1] | keys[2])
    shared, match = eng.exact_screen(paths, paths, k, [0], [0])
    for s in range(3):
        assert [int(x) for x in shared[s]] == [len(keys[s] & keys[i]) for i in range(3)], (k, canonical, s)
        assert int(match[s, 0]) == len(keys[s])
    assert [int(x) for x in shared[3]] == [len(ks) for ks in keys]


# ---- G3. ties to the counting and the emitting paths -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_ties_to_select_and_select_kmers(engine_factory, fixture_paths, k):
    eng = engine_factory()
    ends, _ = cpur.reference(k, True)
    full = 127
    jobs = cpur.group_jobs()
    got = dict(zip(jobs, eng.exact_locate(fixture_paths, k, jobs)))
    found = eng.last_locate_found
    qs = sorted({(a, b) for a, b, _ in jobs})
    fnd = ctypes.c_uint64()
    al, no = np.array([a for a, _ in qs], dtype=np.uint64), np.array([b for _, b in qs], dtype=np.uint64)
    arr = (ctypes.c_char_p * len(fixture_paths))(*[os.fsencode(p) for p in fixture_paths])
    assert eng._lib.dd_exact_select_kmers(eng._ctx, arr, len(fixture_paths), k, al.ctypes.data, no.ctypes.data, len(qs), None, None, 0,
                                          ctypes.byref(fnd)) == 0
    assert found == fnd.value > 0

    def keys_at(words, g):
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        return {ends[g][int(t)] for t in np.flatnonzero(bits)}
    for members in cpur.GROUPS:
        G = sum(1 << i for i in members)
        core, private = int(eng.exact_select(fixture_paths, k, k, [G], [0])[0, 0]), int(eng.exact_select(fixture_paths, k, k, [0], [full ^ G])[0, 0])
        for g in members:
            assert len(keys_at(got[(G, 0, g)], g)) == core, (k, members, g)
        assert len(set().union(*(keys_at(got[(0, full ^ G, g)], g) for g in members))) == private, (k, members)


# ---- G4. records accumulated over passes, ordered once ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 31, 62])
def test_multi_pass_gives_identical_bitmaps(engine_factory, tmp_path, k):
    """17 genomes of 19 kbp, 323 000 occurrences, with a 1 MiB sort budget: a pass holds at most 65 536 k-mers, so at least
    three passes append their records -- more of them, with (0, 0), than a pass's workspace holds -- before the one ordering."""
    eng = engine_factory()
    paths = greedy.write(tmp_path, greedy.related(17, 19_000, 17))
    ntok = [19_001] * 17
    full = (1 << 17) - 1
    G = 0b111
    jobs = [(G, 0, 0), (G, 0, 2), (0, full ^ G, 1), (G, full ^ G, 1), (0, 0, 16), (1 << 5, 0, 5)]
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_locate(paths, k, jobs, ntok=ntok)
    found = eng.last_locate_found
    assert eng.last_sketch_stats()[2] == 1
    os.environ["DD_EXACT_MB"] = "1"
    try:
        many = eng.exact_locate(paths, k, jobs, ntok=ntok)
        passes = eng.last_sketch_stats()[2]
    finally:
        del os.environ["DD_EXACT_MB"]
    assert passes >= 3, (k, passes)
    assert found == eng.last_locate_found > 65_536
    for j, (a, b) in enumerate(zip(one, many)):
        assert a.tobytes() == b.tobytes(), (k, j)
    assert all(one[j].any() for j in (0, 1, 2, 4, 5))      # (the signature of three of 17 related genomes may well be empty)
    bits = np.unpackbits(one[4].view(np.uint8), bitorder="little")         # (0, 0) on a plain record: every token from the k-th base on
    assert np.flatnonzero(bits).tolist() == list(range(k, 19_001))


# ---- G5. the argument rules --------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths):
    from dandd_amd.engine import EngineError
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    paths = fixture_paths[:3]
    ntok = [cpur.index_of(fa)[2] for fa in cpur.genomes()[:3]]
    want = cpur.bitmap([t for t, x in cpur.ends_of(cpur.genomes()[0], 11, True).items()], ntok[0])

    def usable():
        assert np.array_equal(eng.exact_locate(paths, 11, [(1, 0, 0)], ntok=ntok)[0], want)
    for bad, text in ((lambda: eng.exact_locate(paths[:1] * 65, 11, [(1, 0, 0)], ntok=ntok[:1] * 65), "n=65 outside 1..64"),
                      (lambda: eng.exact_locate([], 11, [(1, 0, 0)], ntok=[]), "n=0 outside 1..64"),
                      (lambda: eng.exact_locate(paths, 0, [(1, 0, 0)], ntok=ntok), "outside 1..64"),                 # k = 0
                      (lambda: eng.exact_locate(paths, 65, [(1, 0, 0)], ntok=ntok), "outside 1..64"),                # k = 65
                      (lambda: eng.exact_locate(paths, 11, [], ntok=ntok), "njobs=0 outside 1..1024"),
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, 0)] * 1025, ntok=ntok), "njobs=1025 outside 1..1024"),
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, -1)], ntok=ntok), "job 0: genome -1 outside 0..2"),
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, 0), (1, 0, 3)], ntok=ntok), "job 1: genome 3 outside 0..2"),
                      (lambda: eng.exact_locate(paths, 11, [(8, 0, 0)], ntok=ntok), "job 0: a bit outside 0..2"),    # bit 3 of `all`, n = 3
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, 0), (2, 1 << 63, 1)], ntok=ntok), "job 1: a bit outside 0..2"),
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, 0), (1, 0, 1)], ntok=[ntok[0], ntok[1] + 64, ntok[2]]),
                       f"job 1: .* {(ntok[1] + 63) // 64} expected"),                                               # a wrong off
                      (lambda: eng.exact_locate(paths, 11, [(1, 0, 0)], ntok=[ntok[0] - 64, ntok[1], ntok[2]]),
                       f"job 0: .* {(ntok[0] + 63) // 64} expected")):
        with pytest.raises(EngineError, match=text) as err:
            bad()
        assert err.value.code == DD_EINVAL
        usable()
    # all & none != 0: legal, paints nothing; 1024 jobs; two calls, identical bytes
    zero = eng.exact_locate(paths, 11, [(3, 1, 0), (1, 0, 0)], ntok=ntok)
    assert zero[0].shape == want.shape and not zero[0].any() and np.array_equal(zero[1], want)
    only = eng.exact_locate(paths, 11, [(3, 1, 1)], ntok=ntok)
    assert not only[0].any() and eng.last_locate_found == 0
    big = eng.exact_locate(paths, 11, [(1, 0, 0)] * 1024, ntok=ntok)
    assert all(np.array_equal(w, want) for w in big)
    jobs = cpur.group_jobs(3, [[0, 1], [2]])
    a, b = eng.exact_locate(paths, 33, jobs, ntok=ntok), eng.exact_locate(paths, 33, jobs, ntok=ntok)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and any(x.any() for x in a)
    be = HipExactBackend()
    try:
        assert be.locate_hits([[f"leaf{i}.k11"] for i in range(65)], 11, [(1, 0, 0)]) is None
    finally:
        be.close()


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths):
    eng = engine_factory()
    fas = cpur.genomes()
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    ntok = [cpur.index_of(fa)[2] for fa in fas]
    jobs = cpur.group_jobs()
    for k in (21, 62):
        dev, path = eng.exact_locate_device(ptrs, sizes, k, jobs, ntok), eng.exact_locate(fixture_paths, k, jobs)
        assert any(w.any() for w in path)
        assert all(np.array_equal(x, y) for x, y in zip(dev, path)), k


@pytest.mark.parametrize("kind", ["no record", "no token"])
def test_inputs_without_a_record(engine_factory, torch_cuda, tmp_path, kind):
    """test_gpu_screen's barren universes as the inputs, one (0, 0) job per file: bitmaps of the right length, all zero --
    one word each where the emission ran and found nothing, no word where no input holds a token."""
    paths, _, fas = gpus.barren_files(tmp_path, kind)
    bufs, ptrs, sizes = gpus.on_device(torch_cuda, fas[:3])
    ntok = [cpur.index_of(fa)[2] for fa in fas[:3]]
    assert ntok == ([21] * 3 if kind == "no record" else [0] * 3)
    jobs = [(0, 0, g) for g in range(3)]
    for canonical in (True, False):
        eng = engine_factory(canonical=canonical)
        for k in gpus.BARREN_KS:
            got = eng.exact_locate(paths, k, jobs)
            assert eng.last_locate_found == 0 and len(got) == 3
            assert all(w.shape == ((nt + 63) // 64,) and not w.any() for w, nt in zip(got, ntok)), (kind, canonical, k)
    dev = eng.exact_locate_device(ptrs, sizes, k, jobs, ntok)
    assert eng.last_locate_found == 0 and [w.tolist() for w in dev] == [w.tolist() for w in got]


# ---- G6. the command ------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, sock_dir, torch_cuda):
    """`core --regions` on a real `--exact` tree (HipExactBackend) writes byte for byte the BED files and the index of the CPU
    checker, whose files test_core_regions compares with a per-base coverage; one-shot and through `dandd serve` + the client."""
    from dandd_amd.host import deltatree
    gpu, chk = tmp_path / "gpu", tmp_path / "cpu"
    gpu.mkdir(), chk.mkdir()
    flags = ["--regions", "core", "--regions", "private", "--regions", "signature"]

    def files(d, root):
        out = cpuc._outputs(d)
        return {name: text.replace(str(root).encode(), b"W") for name, text in out.items()}

    def argv_for(root):
        groups = root / "groups.tsv"
        groups.write_text(f"{root / 'data' / 'g0.fasta'}\tleft\ng3.fasta\tright\ng2.fasta\tleft\ng4.fasta\tright\ng1.fasta\talone\n")
        return ["-g", str(groups), *cpuc.WINDOW, *flags]
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(gpu), deltatree, backend=None)
        pkc = cpu.exact_tree(str(chk), deltatree, backend=cpur.RegionBackend)
        a, b = str(gpu / "o"), str(chk / "o")
        deltatree.set_backend_factory(None)
        cpu.run(deltatree, None, "core", argv_for(gpu), pk, a)
        cpu.run(deltatree, cpur.RegionBackend, "core", argv_for(chk), pkc, b)
        got, want = files(a, gpu), files(b, chk)
        assert len([n for n in want if n.endswith(".bed")]) == 3 * 3 and "gold_5_kmc.core_regions.csv" in want
        assert got == want
        groups = [("left", [0, 2]), ("right", [3, 4]), ("alone", [1])]
        summary = {r["group"]: r for r in cpuc._rows(os.path.join(a, "gold_5_kmc.core_groupsummary.csv"))}
        cpur.check_outputs(a, str(gpu / "data"), groups, lambda label, cls: [int(summary[label][f"{cls}_k"])])
    finally:
        deltatree.set_backend_factory(None)
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = ["core", "-d", pk, *argv_for(gpu)]
    sock = os.path.join(sock_dir, "regions.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", *argv, "-o", via], env=cenv, cwd=ROOT, timeout=300,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert files(via, gpu) == got
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()
