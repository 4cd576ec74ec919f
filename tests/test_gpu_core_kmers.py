"""dd_exact_select_kmers on the MI355X: every record -- key, mask and place -- compared with == against membership masks built
in Python from pyref.kmers, at both key widths and on both sides of each boundary between the two ways a k-mer carries its
genome; a query that fills the staging area of every chunk; runs that cross chunks and the all-ones run pad slots share with
T^k; the capacity protocol; multi-pass against single-pass; the device form; the argument rules; the host layer end to end
on a real `--exact` tree; and a size run (thousands of chunks, several per persistent workgroup) checked through identities."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pyref
import test_core as cpuc
import test_core_kmers as cpuk
import test_exact_schedules as cpu
import test_gpu_core as gcore
import test_gpu_exact_schedules as sched

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [1, 5, 21, 28, 29, 32, 33, 48, 56, 57, 60, 61, 64]    # tag in the top byte for 2k <= 56 and 2k - 64 <= 56, in g[] otherwise
NS = [1, 3, 8, 64]
U64 = (1 << 64) - 1
DD_EINVAL = -1


def want_arrays(masks, qs):
    """{k-mer: mask}, [(all, none)] -> the (kmers [m][2], masks [m]) dd_exact_select_kmers owes: test_core_kmers.records_of,
    with one numpy pass per query instead of one Python test per k-mer and query"""
    items = sorted(masks.items())
    m = np.array([v for _, v in items], dtype=np.uint64)
    hit = np.zeros(len(items), dtype=bool)
    for a, b in set(qs):
        hit |= matches(m, a, b)
    return cpuk.arrays_of([items[i] for i in np.flatnonzero(hit)])


def same(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64 and got[0].shape == (len(got[1]), 2), what
    assert len(got[1]) == len(want[1]), (what, len(got[1]), len(want[1]))          # found
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


def ascending(kmers):
    hi, lo = kmers[:, 1], kmers[:, 0]
    return bool(np.all((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))))


def matches(masks, a, b):
    a, b = np.uint64(a), np.uint64(b)
    return ((masks & a) == a) & ((masks & b) == np.uint64(0))


# ---- 1. every record against the masks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_records_match_masks(engine_factory, tmp_path, n, canonical):
    """Two slices of test_gpu_core.queries per k: the last 1024 (at n <= 8 all of them, (0, 0) among them, so every k-mer
    leaves) and the ones behind (0, 0) -- the groups and the random pairs -- which select a part."""
    eng = engine_factory(canonical=canonical)
    fas = sched.genomes(n, sched.LENGTH[n], 1000 + n)
    paths = sched.write(tmp_path, fas)
    qs = gcore.queries(n, n)
    at00 = qs.index((0, 0))
    slices = [qs[-1024:], qs[at00 + 1:]]
    assert all(1 <= len(s) <= 1024 for s in slices)
    at = {q: i for i, q in reversed(list(enumerate(qs)))}
    for k in KS:
        ref = cpuc.masks_of(fas, k, canonical)
        sel = eng.exact_select(paths, k, k, [a for a, _ in qs], [b for _, b in qs])[:, 0]
        for s, part in enumerate(slices):
            got = eng.exact_select_kmers(paths, k, [a for a, _ in part], [b for _, b in part])
            assert eng.last_sketch_stats()[2] == 1                   # (everything at once)
            same(got, want_arrays(ref, part), (n, canonical, k, s))
            for a, b in part:
                assert int(matches(got[1], a, b).sum()) == int(sel[at[(a, b)]]), (n, canonical, k, s, hex(a), hex(b))


# ---- 2. everything: the staging area of every chunk is full ----------------------------------------------------------------
ORDER_KS = [21, 32, 33, 56, 57, 64]    # the records are ordered on the device: one key word up to 32, 2k - 64 bits of hi above


@pytest.mark.parametrize("k", ORDER_KS)
def test_every_distinct_kmer(engine_factory, tmp_path, k):
    eng = engine_factory()
    fas = sched.genomes(1, 4000, 1001)
    paths = sched.write(tmp_path, fas)
    kmers, masks = eng.exact_select_kmers(paths, k, [0], [0])
    want = sorted(set(pyref.kmers(fas[0], k)))
    assert len(masks) == eng.exact_count(paths, k) == len(want)
    assert [int(lo) | int(hi) << 64 for lo, hi in kmers] == want and (k > 32 or not kmers[:, 1].any())
    assert set(int(m) for m in masks) == {1}


# ---- 3. a run across chunks, and the all-ones run ---------------------------------------------------------------------------
def _no_runs(seq, k):
    for base, mid in (("A", "C"), ("T", "G")):
        while base * k in seq:
            seq = seq.replace(base * k, base * (k // 2) + mid + base * (k - k // 2 - 1))
    return seq


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("k", [5, 33])
def test_run_across_chunks(engine_factory, tmp_path, k, canonical):
    """Genomes 0 and 2 hold 5000 bases of poly-A (T with canonical = 0 in the second half of the test): a run of the sorted
    array longer than two chunks of 2048 slots, whose mask the carry brings to its last slot.  A^k leaves once, with mask
    0b101.  canonical = 0: T^k is the all-ones key, the value of the slots the single-pass layout never wrote; it leaves once
    with the genomes that hold it, and not at all when none does."""
    eng = engine_factory(canonical=canonical)
    rng = np.random.default_rng(100 * k + canonical)
    body = [_no_runs("".join("ACGT"[c] for c in rng.integers(0, 4, 600)), 5) for _ in range(5)]
    for base in ("A", "T") if not canonical else ("A",):
        fas = [(">a\n" + body[0] + base * 5000 + body[1] + "\n").encode(),
               (">b\n" + body[0] + "N" + body[1] + "\n>c\n" + body[4] + "\n").encode(),
               (">d\n" + body[2] + "\n>e\n" + base * 5000 + body[3] + "\n").encode()]
        paths = sched.write(tmp_path, fas, tag=base)
        ref = cpuc.masks_of(fas, k, canonical)
        key = 0 if base == "A" else (1 << 2 * k) - 1
        assert ref[key] == 0b101
        for part in ([(0, 0)], [(0b101, 0b010)], [(0b001, 0), (0b100, 0b011)]):
            got = eng.exact_select_kmers(paths, k, [a for a, _ in part], [b for _, b in part])
            assert eng.last_sketch_stats()[2] == 1
            same(got, want_arrays(ref, part), (k, canonical, base, part))
            here = np.flatnonzero((got[0][:, 0] == np.uint64(key & U64)) & (got[0][:, 1] == np.uint64(key >> 64)))
            assert len(here) == 1 and int(got[1][here[0]]) == 0b101
        if base == "A" and not canonical:            # nobody holds T^k: the all-ones run is pad slots only and has no mask
            tk = (1 << 2 * k) - 1
            assert tk not in ref
            kmers, _ = eng.exact_select_kmers(paths, k, [0], [0])
            assert not ((kmers[:, 0] == np.uint64(tk & U64)) & (kmers[:, 1] == np.uint64(tk >> 64))).any()


# ---- 4. the capacity protocol ------------------------------------------------------------------------------------------------
def _raw(eng, paths, k, al, no, nq, kmers, masks, cap, found):
    arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    ptr = lambda a: None if a is None else a.ctypes.data
    return eng._lib.dd_exact_select_kmers(eng._ctx, arr, len(paths), k, ptr(al), ptr(no), nq, ptr(kmers), ptr(masks), cap,
                                          None if found is None else ctypes.byref(found))


@pytest.mark.parametrize("k", ORDER_KS)
def test_capacity_protocol(engine_factory, tmp_path, k):
    eng = engine_factory()
    fas = sched.genomes(3, 2500, 1003)
    paths = sched.write(tmp_path, fas)
    part = [(1, 2), (2, 1)]
    ref = cpuc.masks_of(fas, k, True)
    want = want_arrays(ref, part)
    same(eng.exact_select_kmers(paths, k, [0], [0]), want_arrays(ref, [(0, 0)]), ("every k-mer", k))
    m = len(want[1])
    assert m > 2
    al, no = np.array([a for a, _ in part], dtype=np.uint64), np.array([b for _, b in part], dtype=np.uint64)
    found = ctypes.c_uint64(7)
    assert _raw(eng, paths, k, al, no, 2, None, None, 0, found) == 0 and found.value == m             # a pure count
    kmers, masks = np.zeros((m, 2), dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    found = ctypes.c_uint64(7)
    assert _raw(eng, paths, k, al, no, 2, kmers, masks, m - 1, found) == 0 and found.value == m       # too small: DD_OK, the count
    found = ctypes.c_uint64(7)
    assert _raw(eng, paths, k, al, no, 2, kmers, masks, m, found) == 0 and found.value == m
    same((kmers, masks), want, ("exact cap", k))
    again = (np.zeros((m + 5, 2), dtype=np.uint64), np.zeros(m + 5, dtype=np.uint64))
    assert _raw(eng, paths, k, al, no, 2, *again, m + 5, found) == 0 and found.value == m
    same((again[0][:m], again[1][:m]), want, ("roomy cap", k))
    assert not again[0][m:].any() and not again[1][m:].any()                                       # nothing behind `found`
    # the engine: an exact cap, a cap too small, and the retry of cap=None when the first try is too small
    from dandd_amd.engine import EngineError
    same(eng.exact_select_kmers(paths, k, al, no, cap=m), want, ("engine cap", k))
    with pytest.raises(EngineError, match=f"{m} k-mers") as err:
        eng.exact_select_kmers(paths, k, al, no, cap=m - 1)
    assert err.value.found == m
    first = type(eng).KMERS_FIRST_CAP
    try:
        type(eng).KMERS_FIRST_CAP = 2
        same(eng.exact_select_kmers(paths, k, al, no), want, ("engine retry", k))
    finally:
        type(eng).KMERS_FIRST_CAP = first
    same(eng.exact_select_kmers(paths, k, al, no), want, ("engine default", k))


# ---- 5. passes over parts of the k-mer space ---------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", [3, 8])
def test_multi_pass_gives_identical_arrays(engine_factory, tmp_path, n, canonical):
    """320 kbp in all with a 1 MiB budget (the inputs of test_gpu_exact_schedules' multi-pass test): at least three passes,
    each an arbitrary part of the k-mer space -- the records come back in the order of one pass all the same."""
    eng = engine_factory(canonical=canonical)
    fas = sched.genomes(n, 320_000 // n + 200, 3000 + n)
    paths = sched.write(tmp_path, fas)
    qs = gcore.queries(n, n)
    part = qs[qs.index((0, 0)) + 1:]
    assert "DD_EXACT_MB" not in os.environ
    for k in (5, 21, 31, 48):
        for al, no in (([a for a, _ in part], [b for _, b in part]), ([0], [0])):
            one = eng.exact_select_kmers(paths, k, al, no)
            assert eng.last_sketch_stats()[2] == 1
            os.environ["DD_EXACT_MB"] = "1"
            try:
                many = eng.exact_select_kmers(paths, k, al, no)
                passes = eng.last_sketch_stats()[2]
            finally:
                del os.environ["DD_EXACT_MB"]
            assert passes >= 3, (k, passes)
            assert len(one[1]) > 0 and ascending(one[0])
            assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes(), (n, canonical, k)
        assert len(one[1]) == eng.exact_count(paths, k)                     # (0, 0): every distinct k-mer


# ---- 6. the device form ---------------------------------------------------------------------------------------------------------
def test_device_form_equals_path_form(engine_factory, torch_cuda, tmp_path):
    eng = engine_factory()
    n = 8
    fas = sched.genomes(n, 3000, 77)
    paths = sched.write(tmp_path, fas)
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    qs = gcore.queries(n, 3)
    part = qs[qs.index((0, 0)) + 1:]
    al, no = [a for a, _ in part], [b for _, b in part]
    for k in (8, 21, 31, 62):
        dev, path = eng.exact_select_kmers_device(ptrs, sizes, k, al, no), eng.exact_select_kmers(paths, k, al, no)
        assert len(path[1]) > 0
        assert np.array_equal(dev[0], path[0]) and np.array_equal(dev[1], path[1]), k


# ---- 7. the argument rules ---------------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    fas = sched.genomes(3, 500, 5)
    paths = sched.write(tmp_path, fas)
    want = want_arrays(cpuc.masks_of(fas, 11, True), [(1, 0)])

    def usable():
        same(eng.exact_select_kmers(paths, 11, [1], [0]), want, "after a refused call")
    for bad, text in ((lambda: eng.exact_select_kmers(paths[:1] * 65, 11, [1], [0]), "outside 1..64"),       # n = 65
                      (lambda: eng.exact_select_kmers([], 11, [1], [0]), "outside 1..64"),                   # n = 0
                      (lambda: eng.exact_select_kmers(paths, 0, [1], [0]), "outside 1..64"),                 # k = 0
                      (lambda: eng.exact_select_kmers(paths, 65, [1], [0]), "outside 1..64"),                # k = 65
                      (lambda: eng.exact_select_kmers(paths, 11, [8], [0]), "outside 0..2"),                 # bit 3 of `all`, n = 3
                      (lambda: eng.exact_select_kmers(paths, 11, [1, 2], [0, 1 << 63]), "outside 0..2"),     # bit 63 of `none`
                      (lambda: eng.exact_select_kmers(paths, 11, [], []), "at least one query"),             # nq = 0
                      (lambda: eng.exact_select_kmers(paths, 11, [1] * 1025, [0] * 1025), "at most 1024")):  # nq = 1025
        with pytest.raises(EngineError, match=text) as err:
            bad()
        assert err.value.code == DD_EINVAL
        usable()
    same(eng.exact_select_kmers(paths, 11, [1] * 1024, [0] * 1024), want, "nq = 1024, one k-mer once")
    kmers, masks = eng.exact_select_kmers(paths, 11, [3], [1])                  # all & none != 0: legal, matches nothing
    assert kmers.shape == (0, 2) and masks.shape == (0,)
    # null pointers, straight at the C ABI
    one = np.ones(1, dtype=np.uint64)
    zero = np.zeros(1, dtype=np.uint64)
    kmers, masks, found = np.zeros((4, 2), dtype=np.uint64), np.zeros(4, dtype=np.uint64), ctypes.c_uint64()
    for rc in (_raw(eng, paths, 11, one, zero, 1, kmers, masks, 4, None),        # found
               _raw(eng, paths, 11, one, zero, 1, None, masks, 4, found),        # kmers with cap > 0
               _raw(eng, paths, 11, one, zero, 1, kmers, None, 4, found),        # masks with cap > 0
               _raw(eng, paths, 11, None, zero, 1, kmers, masks, 4, found),
               _raw(eng, paths, 11, one, None, 1, kmers, masks, 4, found)):
        assert rc == DD_EINVAL and "null" in eng._lib.dd_last_error().decode()
        usable()
    be = HipExactBackend()
    try:
        assert be.select_kmers([[f"leaf{i}.k11"] for i in range(65)], 11, [1], [0], 10) is None
    finally:
        be.close()


# ---- 8. the host layer end to end -----------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, sock_dir, torch_cuda):
    """`core --kmers` on a real `--exact` tree (HipExactBackend) writes byte for byte the files of the CPU checker, one-shot
    and through `dandd serve` + the client."""
    from dandd_amd.host import deltatree
    gpu, chk = tmp_path / "gpu", tmp_path / "cpu"
    gpu.mkdir(), chk.mkdir()
    flags = ["--kmers", "core", "--kmers", "private", "--kmers", "signature", "--kmers-k", "9", "--kmers-k", "12"]

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
        pkc = cpu.exact_tree(str(chk), deltatree, backend=cpuk.KmerBackend)
        a, b = str(gpu / "o"), str(chk / "o")
        deltatree.set_backend_factory(None)
        cpu.run(deltatree, None, "core", argv_for(gpu), pk, a)
        cpu.run(deltatree, cpuk.KmerBackend, "core", argv_for(chk), pkc, b)
        got, want = files(a, gpu), files(b, chk)
        assert len([n for n in want if n.endswith(".fasta")]) == 3 * 3 * 2 and "gold_5_kmc.core_kmers.csv" in want
        assert got == want
    finally:
        deltatree.set_backend_factory(None)
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = ["core", "-d", pk, *argv_for(gpu)]
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", *argv, "-o", one], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert files(one, gpu) == got
    sock = os.path.join(sock_dir, "kmers.sock")
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


# ---- 9. one size run ------------------------------------------------------------------------------------------------------------
def test_size_16_genomes_1mbp(engine_factory, torch_cuda):
    """16 x 1 Mbp synthetic genomes at k = 21: 7 800 chunks of sorted k-mers, several per persistent workgroup, which no small
    case reaches.  No Python sets at this size: the keys ascend strictly, every mask satisfies a query, the masks that match
    each query are as many as dd_exact_select counts, and (0, 0) finds dd_exact_count k-mers."""
    from dandd_amd.engine import synth_size
    eng = engine_factory()
    torch = torch_cuda
    n, nb, k = 16, 1_000_000, 21
    bufs, sizes = [], []
    for gi in range(n):
        size = synth_size(nb, 4)
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(0xD4ADD, gi, nb, 4, t.data_ptr())
        bufs.append(t)
        sizes.append(size)
    eng.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    full = (1 << n) - 1
    groups = [0xF << 4 * g for g in range(4)]
    qs = [q for G in groups for q in ((G, 0), (0, full ^ G), (G, full ^ G))]
    al, no = [a for a, _ in qs], [b for _, b in qs]
    sel = eng.exact_select_device(ptrs, sizes, k, k, al, no)[:, 0]
    kmers, masks = eng.exact_select_kmers_device(ptrs, sizes, k, al, no)
    print(f"\n16 x 1 Mbp, k = {k}: {len(masks)} k-mers match the 12 queries of four groups of four")
    assert len(masks) > 0 and ascending(kmers) and not kmers[:, 1].any()
    hit = np.zeros(len(masks), dtype=bool)
    for q, (a, b) in enumerate(qs):
        mine = matches(masks, a, b)
        assert int(mine.sum()) == int(sel[q]), (q, hex(a), hex(b))
        hit |= mine
    assert hit.all()
    lib, found = eng._lib, ctypes.c_uint64()
    zero = np.zeros(1, dtype=np.uint64)
    rc = lib.dd_exact_select_kmers_device(eng._ctx, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_size_t * n)(*sizes), n, k, zero.ctypes.data,
                                          zero.ctypes.data, 1, None, None, 0, ctypes.byref(found))
    assert rc == 0 and found.value == eng.exact_count_device(ptrs, sizes, k)
