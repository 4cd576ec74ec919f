"""dd_exact_patterns on the MI355X: the distinct membership masks and their multiplicities from the patterns accumulator of
dd_exact_sched.hip and the merges of dd_exact_patterns.hip, compared with == against collections.Counter over
test_core_regions.reference (the 7-input fixture, every tag mode and key width), against a numpy table of random genomes
where the workgroups' tables spill, write masks through singly and collide, across passes, and against the other
accumulators of the same sort (count, spectrum, select, subsets) at 16 x 1 Mbp and at a size where the default table
spills; the argument rules; and the command on a real exact tree."""
import collections
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_core_regions as cpur
import test_exact_schedules as cpu
import test_gpu_exact_greedy as greedy
import test_patterns as cpup

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [11, 28, 29, 32, 33, 60, 61, 64]     # test_gpu_core_regions': both tag modes, 64- and 128-bit keys
KS_NOCANON = [11, 32, 33, 64]
DD_EINVAL = -1
SEED = 20261020


class knob:
    """an environment variable of the library for the length of a with block"""

    def __init__(self, name, value):
        self.name, self.value = name, str(value)

    def __enter__(self):
        assert self.name not in os.environ
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        del os.environ[self.name]


def rows(got):
    masks, counts, found = got
    assert masks.dtype == np.uint64 and counts.dtype == np.uint64 and masks.shape == counts.shape
    return list(zip(masks.tolist(), counts.tolist())), found


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- a numpy table of random genomes: computed once per shape, never changed -------------------------------------------------
def codes_of(n, length, seed=SEED):
    return np.random.default_rng(seed).integers(0, 4, (n, length))


def fasta_of(codes, name):
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode()
    return (f">{name}\n" + "".join(text[j:j + 80] + "\n" for j in range(0, len(text), 80))).encode()


def kmers_of(codes, k):
    """the distinct canonical k-mers (k <= 31) of one record, as uint64"""
    m = len(codes) - k + 1
    f, r = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    for j in range(k):
        c = codes[j:j + m].astype(np.uint64)
        f = (f << np.uint64(2)) | c
        r |= (np.uint64(3) - c) << np.uint64(2 * j)
    return np.unique(np.minimum(f, r))


def table_of(per_genome, bits):
    """[distinct k-mers of genome i], the bit each sets -> ([(mask, count)] in the order of the ABI, distinct k-mers)"""
    universe = np.unique(np.concatenate(per_genome))
    masks = np.zeros(len(universe), dtype=np.uint64)
    for kmers, bit in zip(per_genome, bits):
        masks[np.searchsorted(universe, kmers)] |= np.uint64(1 << bit)
    um, uc = np.unique(masks, return_counts=True)
    order = np.lexsort((um, -uc.astype(np.int64)))
    return list(zip(um[order].tolist(), uc[order].tolist())), len(universe)


@functools.lru_cache(maxsize=None)
def random_case(n, k):
    codes = codes_of(n, 8000)
    return [fasta_of(codes[i], f"r{i}") for i in range(n)], table_of([kmers_of(codes[i], k) for i in range(n)], range(n))


def popcounts(masks):
    m = masks.astype(np.uint64)
    m = m - ((m >> np.uint64(1)) & np.uint64(0x5555555555555555))
    m = (m & np.uint64(0x3333333333333333)) + ((m >> np.uint64(2)) & np.uint64(0x3333333333333333))
    m = (m + (m >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((m * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def spectrum_of(masks, counts, n):
    return np.bincount(popcounts(masks), weights=counts.astype(np.float64), minlength=n + 1).astype(np.uint64)   # (sums below 2^53)


def select_of(masks, counts, a, b):
    hit = ((masks & np.uint64(a)) == np.uint64(a)) & ((masks & np.uint64(b)) == np.uint64(0))
    return int(counts[hit].sum())


@pytest.fixture(scope="module")
def fixture_paths(tmp_path_factory):
    return cpur.write_genomes(tmp_path_factory.mktemp("patterns_universe"))


# ---- 1. every row against the sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical,k", [(True, k) for k in KS] + [(False, k) for k in KS_NOCANON])
def test_every_row_equals_the_sets(engine_factory, fixture_paths, canonical, k):
    eng = engine_factory(canonical=canonical)
    _, masks = cpur.reference(k, canonical)
    want = cpup.ordered(collections.Counter(masks.values()))
    got = eng.exact_patterns(fixture_paths, k)
    assert eng.last_sketch_stats()[2] == 1
    assert rows(got) == (want, len(want)), (k, canonical)
    stats = eng.last_patterns_stats
    assert stats[0] == len(masks) == sum(c for _, c in want) and stats[1] >= len(want) and stats[2] == 0 == stats[3]
    # cap = 0: a pure count; cap = 3: the first three rows of the full answer; two calls: identical bytes
    none = eng.exact_patterns(fixture_paths, k, cap=0)
    assert none[0].size == 0 == none[1].size and none[2] == len(want) > 3
    assert rows(eng.exact_patterns(fixture_paths, k, cap=3)) == (want[:3], len(want))
    assert same_bytes(got, eng.exact_patterns(fixture_paths, k))
    # the fixture does what it is for: g4 is g0, g6 is empty, and at most k the 40 bases of g5 hold something
    assert all(m >> 6 == 0 and (m & 1) == (m >> 4 & 1) for m, _ in want) and any(m >> 5 & 1 for m, _ in want) == (k <= 40)


# ---- 2. the spill path at the smallest shape that reaches it --------------------------------------------------------------------
@pytest.mark.parametrize("k,kmers,patterns", [(7, 8192, 7132), (8, 32145, 8617)])
def test_a_small_table_spills(engine_factory, tmp_path, k, kmers, patterns):
    """16 random genomes x 8 000 bases: at k = 7 every canonical 7-mer occurs, in 7 132 patterns of which the largest holds 7
    k-mers -- some 130 masks per chunk of the sort, nearly all of them ties --, at k = 8 some 510 per chunk.  A table of 64
    slots cannot hold a chunk's masks: it flushes, and masks leave singly."""
    eng = engine_factory()
    fas, (want, distinct) = random_case(16, k)
    assert (distinct, len(want)) == (kmers, patterns) and (k != 7 or want[0][1] == 7)
    paths = greedy.write(tmp_path, fas)
    with knob("DD_PATTERNS_SLOTS", 64):
        small = eng.exact_patterns(paths, k)
        stats = eng.last_patterns_stats
        assert rows(small) == (want, len(want))
        assert same_bytes(small, eng.exact_patterns(paths, k))
    assert stats[0] == distinct and stats[2] > 0 and stats[1] >= len(want) and stats[1] <= distinct
    assert same_bytes(small, eng.exact_patterns(paths, k))          # the default table
    assert eng.last_patterns_stats[2] == 0


# ---- 3. wide masks, no pattern repeated ------------------------------------------------------------------------------------------
def test_64_genomes_every_pattern_once(engine_factory, tmp_path):
    eng = engine_factory()
    fas, (want, distinct) = random_case(64, 7)
    assert distinct == len(want) == 8192 and all(c == 1 for _, c in want)
    paths = greedy.write(tmp_path, fas)
    with knob("DD_PATTERNS_SLOTS", 64):
        small = eng.exact_patterns(paths, 7)
    for got in (small, eng.exact_patterns(paths, 7)):
        table, found = rows(got)
        assert found == 8192 and table == want and [m for m, _ in table] == sorted(m for m, _ in table)
    seen = 0
    for m, _ in want:
        seen |= m
    assert seen == (1 << 64) - 1


# ---- 4. masks that differ in their top bits only -----------------------------------------------------------------------------------
def test_genomes_on_the_top_bits(engine_factory, tmp_path):
    """64 inputs of which only 48..63 hold anything: every mask agrees in its 48 low bits"""
    eng = engine_factory()
    codes = codes_of(16, 8000)
    want, distinct = table_of([kmers_of(codes[i], 8) for i in range(16)], range(48, 64))
    fas = [b""] * 48 + [fasta_of(codes[i], f"r{i}") for i in range(16)]
    paths = greedy.write(tmp_path, fas)
    assert all(m & ((1 << 48) - 1) == 0 for m, _ in want) and len(want) == 8617
    for slots in (64, 256, None):
        if slots is None:
            got = eng.exact_patterns(paths, 8)
        else:
            with knob("DD_PATTERNS_SLOTS", slots):
                got = eng.exact_patterns(paths, 8)
        assert rows(got) == (want, len(want)) and eng.last_patterns_stats[0] == distinct, slots


# ---- 5. passes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 31, 62])
def test_multi_pass_gives_the_same_table(engine_factory, tmp_path, k):
    eng = engine_factory()
    paths = greedy.write(tmp_path, greedy.related(17, 19_000, 17))
    assert "DD_EXACT_MB" not in os.environ
    one = eng.exact_patterns(paths, k)
    assert eng.last_sketch_stats()[2] == 1
    first = eng.last_patterns_stats
    with knob("DD_EXACT_MB", 1):
        many = eng.exact_patterns(paths, k)
        passes = eng.last_sketch_stats()[2]
        with knob("DD_PATTERNS_SLOTS", 64):
            spilled = eng.exact_patterns(paths, k)
    assert passes >= 2, (k, passes)
    assert same_bytes(one, many) and same_bytes(one, spilled)
    table, found = rows(one)
    assert found == len(table) > 100 and sum(c for _, c in table) == first[0] == eng.exact_count(paths, k)
    assert table[0][0] == (1 << 17) - 1 or bin(table[0][0]).count("1") == 1      # related genomes: the core or a private set leads


# ---- 6. the other accumulators of the same sort ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def related_paths(tmp_path_factory):
    return greedy.write(tmp_path_factory.mktemp("patterns_related"), greedy.related(16, 1_000_000, 6))


@pytest.mark.parametrize("k", [21, 33])
def test_the_table_gives_every_other_count(engine_factory, related_paths, k):
    """16 related genomes x 1 Mbp: some 7 800 chunks, 15 per workgroup -- the regime of test_size_16_genomes_5mbp"""
    from dandd_amd.engine import exact_subsets_from_hist
    eng = engine_factory()
    n, paths = 16, related_paths
    full = (1 << n) - 1
    masks, counts, found = eng.exact_patterns(paths, k)
    stats = eng.last_patterns_stats
    assert found == len(masks) == len(set(masks.tolist())) and (masks != 0).all() and (masks <= full).all()
    assert int(counts.sum()) == stats[0] == eng.exact_count(paths, k)
    assert spectrum_of(masks, counts, n).tolist() == eng.exact_spectrum(paths, k, k)[:, 0].tolist()
    rng = np.random.default_rng(k)
    qs = [(0, 0), (full, 0), (1, full ^ 1), (0, 1), (3, 0), (0b1010, 0b0101)] + \
        [(int(a), int(b) & ~int(a)) for a, b in zip(rng.integers(0, full + 1, size=6), rng.integers(0, full + 1, size=6))]
    sel = eng.exact_select(paths, k, k, [a for a, _ in qs], [b for _, b in qs])[:, 0]
    assert [select_of(masks, counts, a, b) for a, b in qs] == sel.tolist() and sel[0] == stats[0] and sel[1] > 0
    hist = np.zeros(1 << n, dtype=np.uint64)
    hist[masks.astype(np.int64)] = counts
    assert exact_subsets_from_hist(hist, n).tolist() == eng.exact_subsets(paths, k, k)[:, 0].tolist()
    order = np.lexsort((masks, -counts.astype(np.int64)))
    assert (order == np.arange(len(masks))).all()


# ---- 7. the default table spills ---------------------------------------------------------------------------------------------------
def test_the_default_table_spills_at_size(engine_factory, torch_cuda):
    """64 random genomes x 300 kbp at k = 12: 19 M occurrences over the 8.4 M canonical 12-mers, 2.3 genomes to a k-mer on
    average.  A workgroup reduces 1 / 512 of the sort, some 14 700 k-mers; the 43 744 masks of one, two or three bits alone
    are more than its 4 096 slots hold, and the fifth of the k-mers that four genomes or more hold (Poisson, mean 2.3) bring
    over a million masks that hardly repeat: every workgroup flushes a full table several times."""
    eng = engine_factory()
    torch = torch_cuda
    n, nb, k = 64, 300_000, 12
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    head = torch.tensor(list(b">r\n"), dtype=torch.uint8, device="cuda")
    bufs = [torch.cat([head, letters[torch.randint(0, 4, (nb,), device="cuda", generator=gen)],
                       torch.full((17,), 10, dtype=torch.uint8, device="cuda")]) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs, sizes = [b.data_ptr() for b in bufs], [nb + 4] * n
    assert "DD_PATTERNS_SLOTS" not in os.environ
    masks, counts, found = eng.exact_patterns_device(ptrs, sizes, k)
    stats = eng.last_patterns_stats
    assert stats[2] >= 512 and found == len(masks) > 1_000_000, stats
    assert int(counts.sum()) == stats[0] == eng.exact_count_device(ptrs, sizes, k)
    assert spectrum_of(masks, counts, n).tolist() == eng.exact_spectrum_device(ptrs, sizes, k, k)[:, 0].tolist()
    full = (1 << n) - 1
    qs = [(0, 0), (1, 0), (0, 1), (1 << 63, 0), (0, full ^ 0xFF), (0x8000000000000001, 2), (3 << 31, 0), (0, 0xFFFF << 24)]
    sel = eng.exact_select_device(ptrs, sizes, k, k, [a for a, _ in qs], [b for _, b in qs])[:, 0]
    assert [select_of(masks, counts, a, b) for a, b in qs] == sel.tolist()
    with knob("DD_PATTERNS_SLOTS", 64):
        small = eng.exact_patterns_device(ptrs, sizes, k, cap=found)
        assert eng.last_patterns_stats[2] > stats[2]
    assert same_bytes((masks, counts, found), small)


# ---- 8. the argument rules ----------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, fixture_paths):
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    lib = eng._lib
    lib.dd_last_error.restype = ctypes.c_char_p
    _, ref = cpur.reference(11, True)
    want = cpup.ordered(collections.Counter(ref.values()))

    def call(paths=fixture_paths, k=11, cap=4, null=()):
        n = len(paths)
        pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
        masks, counts = np.full(max(cap, 1), 77, dtype=np.uint64), np.full(max(cap, 1), 77, dtype=np.uint64)
        found, stats = ctypes.c_uint64(77), np.full(4, 77, dtype=np.uint64)
        rc = lib.dd_exact_patterns(eng._ctx, None if "paths" in null else pa, n, k, None if "masks" in null else masks.ctypes.data,
                                   None if "counts" in null else counts.ctypes.data, cap, None if "found" in null else ctypes.byref(found),
                                   None if "stats" in null else stats.ctypes.data)
        return rc, masks, counts, found.value, stats, lib.dd_last_error().decode()

    def usable():
        rc, masks, counts, found, stats, _ = call()
        assert rc == 0 and found == len(want) and list(zip(masks.tolist(), counts.tolist())) == want[:4] and stats[0] == len(ref)
    usable()
    for kw, text in ((dict(paths=[]), "n=0 outside 1..64"), (dict(paths=fixture_paths[:1] * 65), "n=65 outside 1..64"),
                     (dict(null=("paths",)), "null argument"), (dict(null=("found",)), "null argument"),
                     (dict(k=0), "outside 1..64"), (dict(k=65), "outside 1..64"),
                     (dict(null=("masks",)), "null argument"), (dict(null=("counts",)), "null argument")):
        rc, masks, counts, found, stats, err = call(**kw)
        assert rc == DD_EINVAL and text in err, (kw, rc, err)
        assert (masks == 77).all() and (counts == 77).all() and found == 77 and (stats == 77).all(), kw     # the outputs are untouched
        usable()
    # the order of exact_args: n before the null pointers, those before k
    assert "n=0" in call(paths=[], k=0, null=("found",))[5] and "null argument" in call(k=0, null=("found",))[5]
    # null arrays with cap = 0 and null stats: a pure count
    rc, masks, counts, found, stats, _ = call(cap=0, null=("masks", "counts", "stats"))
    assert rc == 0 and found == len(want) and (stats == 77).all()
    # the knob's own rule
    for bad in ("63", "100", "16384", "x"):
        with knob("DD_PATTERNS_SLOTS", bad):
            rc, _, _, found, _, err = call()
            assert rc == DD_EINVAL and "DD_PATTERNS_SLOTS" in err and found == 77, bad
    # no input holds a k-mer: nothing found, every stat 0
    got = eng.exact_patterns([fixture_paths[6], fixture_paths[6]], 11)
    assert got[0].size == 0 and got[2] == 0 and eng.last_patterns_stats == (0, 0, 0, 0)
    got = eng.exact_patterns([fixture_paths[5]], 41)
    assert got[2] == 0 and eng.last_patterns_stats == (0, 0, 0, 0)
    be = HipExactBackend()
    try:
        assert be.pattern_counts([[f"leaf{i}.k11"] for i in range(65)], 11, None) is None
    finally:
        be.close()


def test_device_form_equals_path_form(engine_factory, torch_cuda, fixture_paths):
    eng = engine_factory()
    fas = list(cpur.genomes())
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    for k in (21, 62):
        dev, path = eng.exact_patterns_device(ptrs, sizes, k), eng.exact_patterns(fixture_paths, k)
        assert path[2] > 3 and same_bytes(dev, path), k


# ---- 9. the command -----------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, torch_cuda):
    """`patterns` on a real `--exact` tree (HipExactBackend), as a process of its own and through serve / client: the CSVs
    equal the tables test_patterns computes from the files' text, which are what its checker backend writes."""
    from dandd_amd.host import deltatree
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(tmp_path), deltatree, backend=None)
    finally:
        deltatree.set_backend_factory(None)
    data = str(tmp_path / "data")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = ["patterns", "-d", pk, "-k", "9", "-k", "12", "-k", "33", "--splits", "--top", "7"]
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", *argv, "-o", out], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = cpup.read_csvs(out)
    assert got == cpup.tables(cpup.golden_universe(data), [9, 12, 33], top=7, splits=True)
    assert len(got["patterns"]) == 3 * 7 and len(got["splits"]) > 0
    sock = str(tmp_path / "p.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        via = str(tmp_path / "srv")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", *argv, "-o", via], env=dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1"),
                           cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert cpup.read_csvs(via) == got
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()
