"""dd_exact_wide_pairwise / _progressive / _leave_out on the MI355X: the union schedules for up to 255 genomes from one sort
per k.  Every count compared with == against tests/wide_ref.py (Python sets of pyref.kmers): every row width (n = 1 .. 255),
both ways a k-mer carries its genome at both key widths, the narrow entries byte for byte where they apply, a run that spans
several chunks with bits in every word of the row, T^k in the highest genome beside the unwritten slots, passes, the device
forms, the limits, the host layer end to end on an exact tree of 70 genomes, and a size run (printed, correctness asserted)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import hostcheck
import test_exact_schedules as cpu
import test_exact_wide as host_cpu
import test_gpu_exact_schedules as narrow
from wide_ref import WideRef

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NS = [1, 2, 64, 65, 128, 129, 255]
LENGTH = {1: 400, 2: 400, 64: 300, 65: 300, 128: 200, 129: 200, 255: 200}      # bases per genome
RANGES = [(11, 11), (21, 21), (31, 31), (33, 33), (63, 63), (30, 33), (61, 64)]

_REFS = {}


def reference(n, canonical):
    """the genomes of a case and their reference, made once and shared by the cases that need them"""
    key = (n, bool(canonical))
    if key not in _REFS:
        fas = narrow.genomes(n, LENGTH[n], 5000 + n)
        _REFS[key] = (fas, WideRef(fas, canonical))
    return _REFS[key]


def check_wide(eng, paths, ref, n, kmin, kmax, seed):
    """all three wide schedules over kmin..kmax against the reference; -> the arrays"""
    K = kmax - kmin + 1
    got = {}
    pw = got["pairwise"] = eng.exact_wide_pairwise(paths, kmin, kmax)
    assert pw.shape == (n, n, K) and pw.dtype == np.uint64
    assert np.array_equal(pw, ref.pairwise(kmin, kmax)), ("pairwise", n, kmin, kmax)
    ords = narrow.orderings(n, seed)                                     # 7 orderings
    pr = got["progressive"] = eng.exact_wide_progressive(paths, kmin, kmax, ords)
    assert pr.shape == (len(ords), n, K) and pr.dtype == np.uint64
    assert np.array_equal(pr, ref.progressive(kmin, kmax, ords)), ("progressive", n, kmin, kmax)
    for gi, group in enumerate(narrow.groupings(n)):                     # singletons; two groups plus ungrouped leaves
        G = max(group) + 1
        lo = got[f"leave_out{gi}"] = eng.exact_wide_leave_out(paths, kmin, kmax, group, G)
        assert lo.shape == (G + 1, K) and lo.dtype == np.uint64
        assert np.array_equal(lo, ref.leave_out(kmin, kmax, group, G)), ("leave_out", n, kmin, kmax, gi)
        assert np.array_equal(lo[G], pr[0, n - 1])                       # M, twice
    return got


# ---- 1. against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("krange", RANGES, ids=[f"k{a}-{b}" for a, b in RANGES])
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_wide_schedules_match_the_reference(engine_factory, tmp_path, n, canonical, krange):
    eng = engine_factory(canonical=canonical)
    fas, ref = reference(n, canonical)
    paths = narrow.write(tmp_path, fas)
    check_wide(eng, paths, ref, n, *krange, seed=n)
    assert eng.last_sketch_stats()[2] == 1                               # (everything at once)


# ---- 2. narrow equals wide ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", [1, 3, 33, 64])
def test_wide_entries_equal_the_narrow_ones(engine_factory, tmp_path, n, canonical):
    eng = engine_factory(canonical=canonical)
    paths = narrow.write(tmp_path, narrow.genomes(n, narrow.LENGTH[n] if n in narrow.LENGTH else 400, 6000 + n))
    ords = narrow.orderings(n, n)
    for kmin, kmax in RANGES:
        a, b = eng.exact_pairwise(paths, kmin, kmax), eng.exact_wide_pairwise(paths, kmin, kmax)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), ("pairwise", kmin, kmax)
        a, b = eng.exact_progressive(paths, kmin, kmax, ords), eng.exact_wide_progressive(paths, kmin, kmax, ords)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), ("progressive", kmin, kmax)
        for group in narrow.groupings(n):
            a = eng.exact_leave_out(paths, kmin, kmax, group, max(group) + 1)
            b = eng.exact_wide_leave_out(paths, kmin, kmax, group, max(group) + 1)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), ("leave_out", kmin, kmax)


# ---- 3. a run across several chunks, bits in every word -----------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
def test_a_run_across_chunks_with_bits_in_every_word(engine_factory, tmp_path, canonical):
    """200 genomes hold A^40 and one holds A^6000: at k = 11 the run of A^k is about 12 000 slots long -- six chunks of 2048,
    at least one of them without a head -- and collects bits of all four words of its row on the way.  Three ordinary genomes
    beside them, so that the row of A^k is not the only one."""
    k = 11
    eng = engine_factory(canonical=canonical)
    fas = [f">a{i}\n{'A' * 40}\n".encode() for i in range(200)] + [b">long\n" + b"A" * 6000 + b"\n"]
    fas += [f for f in narrow.genomes(4, 300, 77) if f]
    n = len(fas)
    assert n == 204
    ref = WideRef(fas, canonical)
    assert all(0 in s for s in ref.sets(k)[:201])                       # (A^k is key 0, in every one of the first 201)
    got = check_wide(eng, narrow.write(tmp_path, fas), ref, n, k, k, seed=3)
    assert int(got["pairwise"][0, 199, 0]) == int(got["pairwise"][5, 5, 0]) == 1
    assert int(got["leave_out0"][200, 0]) == int(got["leave_out0"][n, 0])   # (without the long genome: nothing is lost)


# ---- 4. T^k and the slots nothing was written to ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 21, 31, 40, 63])
def test_all_t_kmer_in_the_highest_genome_shares_its_run_with_unwritten_slots(engine_factory, tmp_path, k):
    """canonical = 0: T^k survives as the all-ones key, the value the unwritten slots of the single-pass layout hold (with the
    genome 0xFF, which sets no bit).  Genome 254 of 255 holds the T run: T^k is counted once, and only in the unions that
    hold genome 254."""
    n = 255
    eng = engine_factory(canonical=False)
    rng = np.random.default_rng(k)
    body = ["".join("ACGT"[c] for c in rng.integers(0, 4, 300)).replace("T" * 5, "TTGTT") for _ in range(3)]
    with_t = (">t\n" + body[0] + "T" * 100 + body[1] + "\n").encode()
    plain = [(">n\n" + body[0] + "N" + body[1] + "\n").encode(), (">m\n" + body[2] + "\n").encode()]
    fas = [plain[i % 2] for i in range(n - 1)] + [with_t]
    ref = WideRef(fas, False)
    tk = (1 << (2 * k)) - 1
    assert tk in ref.sets(k)[n - 1] and not any(tk in s for s in ref.sets(k)[:n - 1])
    got = check_wide(eng, narrow.write(tmp_path, fas), ref, n, k, k, seed=k)
    assert eng.last_sketch_stats()[2] == 1
    pw, lo = got["pairwise"][:, :, 0], got["leave_out0"][:, 0]
    both, every = ref.count([0, 1], k), ref.count(range(n), k)
    assert tk in set().union(*ref.sets(k)) and every > both              # (what genome 254 adds holds T^k)
    assert int(pw[n - 1, n - 1]) == len(ref.sets(k)[n - 1]) and int(pw[0, 1]) == int(pw[2, 3]) == both
    assert int(lo[n]) == every and int(lo[n - 1]) == both                # all; all but genome 254: T^k gone, counted nowhere


# ---- 5. passes over parts of the k-mer space ----------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
def test_multi_pass_gives_identical_arrays(engine_factory, tmp_path, canonical):
    """130 genomes of 2 500 bases with a 1 MiB budget: at least three passes, the arrays of the single pass, and a few unions
    of every schedule the reference's count."""
    n = 130
    eng = engine_factory(canonical=canonical)
    fas = narrow.genomes(n, 2500, 7000)
    paths = narrow.write(tmp_path, fas)
    ref = WideRef(fas, canonical)
    ords, group = narrow.orderings(n, n), narrow.groupings(n)[1]
    assert "DD_EXACT_MB" not in os.environ
    for kmin, kmax in [(21, 21), (31, 31), (33, 33), (63, 63)]:
        calls = [("pairwise", lambda: eng.exact_wide_pairwise(paths, kmin, kmax)),
                 ("progressive", lambda: eng.exact_wide_progressive(paths, kmin, kmax, ords)),
                 ("leave_out", lambda: eng.exact_wide_leave_out(paths, kmin, kmax, group, 2))]
        for what, call in calls:
            one = call()
            assert eng.last_sketch_stats()[2] == 1
            os.environ["DD_EXACT_MB"] = "1"
            try:
                many = call()
                passes = eng.last_sketch_stats()[2]
            finally:
                del os.environ["DD_EXACT_MB"]
            print(f"n={n} canonical={canonical} k={kmin} {what}: {passes} passes")
            assert passes >= 3, (what, kmin, passes)
            assert np.array_equal(one, many), (what, kmin)
            if what == "pairwise":
                for i, j in [(0, 0), (0, n - 2), (64, 127), (1, 128)]:
                    assert int(many[i, j, 0]) == ref.count({i, j}, kmin), (kmin, i, j)
            if what == "progressive":
                for o, j in [(0, 70), (1, 2), (4, n - 1)]:
                    assert int(many[o, j, 0]) == ref.count(ords[o][:j + 1], kmin), (kmin, o, j)
            if what == "leave_out":
                for g in range(3):
                    assert int(many[g, 0]) == ref.count([i for i in range(n) if group[i] != g], kmin), (kmin, g)


# ---- 6. / 7. device forms; two calls ------------------------------------------------------------------------------------
def test_device_forms_equal_path_forms_and_two_calls_agree(engine_factory, torch_cuda, tmp_path):
    eng = engine_factory()
    n = 70
    fas = narrow.genomes(n, 300, 78)
    paths = narrow.write(tmp_path, fas)
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    ords, group = narrow.orderings(n, 3), narrow.groupings(n)[1]
    for kmin, kmax in [(21, 21), (30, 33), (61, 64)]:
        pw, pr, lo = (eng.exact_wide_pairwise(paths, kmin, kmax), eng.exact_wide_progressive(paths, kmin, kmax, ords),
                      eng.exact_wide_leave_out(paths, kmin, kmax, group))
        assert eng.exact_wide_pairwise_device(ptrs, sizes, kmin, kmax).tobytes() == pw.tobytes()
        assert eng.exact_wide_progressive_device(ptrs, sizes, kmin, kmax, ords).tobytes() == pr.tobytes()
        assert eng.exact_wide_leave_out_device(ptrs, sizes, kmin, kmax, group).tobytes() == lo.tobytes()
        assert eng.exact_wide_pairwise(paths, kmin, kmax).tobytes() == pw.tobytes()
        assert eng.exact_wide_progressive(paths, kmin, kmax, ords).tobytes() == pr.tobytes()
        assert eng.exact_wide_leave_out(paths, kmin, kmax, group).tobytes() == lo.tobytes()


# ---- 8. limits -------------------------------------------------------------------------------------------------------------
def test_limits_and_argument_rules(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    one = narrow.write(tmp_path, narrow.genomes(1, 300, 9))
    three = narrow.write(tmp_path, narrow.genomes(3, 300, 10), tag="t")
    for many in ([], one * 256):
        n = len(many)
        with pytest.raises(EngineError, match="outside 1..255"):
            eng.exact_wide_pairwise(many, 11, 11)
        with pytest.raises(EngineError, match="outside 1..255"):
            eng.exact_wide_progressive(many, 11, 11, [list(range(max(n, 1)))])
        with pytest.raises(EngineError, match="outside 1..255"):
            eng.exact_wide_leave_out(many, 11, 11, list(range(max(n, 1))))
    assert eng.exact_wide_pairwise(one * 255, 11, 11).shape == (255, 255, 1)
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_wide_pairwise(three, 0, 11)
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_wide_pairwise(three, 60, 65)
    with pytest.raises(EngineError, match="not a permutation"):
        eng.exact_wide_progressive(three, 11, 11, [[0, 1, 1]])
    with pytest.raises(EngineError, match="outside 0..2"):
        eng.exact_wide_progressive(three, 11, 11, [[0, 1, 3]])
    with pytest.raises(EngineError, match="outside -1..0"):
        eng.exact_wide_leave_out(three, 11, 11, [0, 1, -1], 1)
    with pytest.raises(EngineError, match="holds every leaf"):
        eng.exact_wide_leave_out(three, 11, 11, [0, 0, 0], 1)
    with pytest.raises(EngineError, match="holds every leaf"):
        eng.exact_wide_leave_out(one * 200, 11, 11, [0] * 200, 1)
    be = HipExactBackend()
    try:
        rows = [[f"leaf{i}.k11"] for i in range(256)]
        assert be.wide_pairwise_cards(rows) is None
        assert be.wide_progressive_cards(rows, [list(range(256))]) is None
        assert be.wide_leave_out_cards(rows, list(range(256))) is None
        assert be.pairwise_cards(rows[:65]) is None
    finally:
        be.close()


# ---- 9. the host layer end to end ---------------------------------------------------------------------------------------
def test_cli_end_to_end_on_a_tree_of_70(tmp_path, sock_dir, torch_cuda, monkeypatch):
    """`kij --jaccard`, `progressive -n 3` and `deltadelta` on a real `--exact` tree of 70 genomes (HipExactBackend: the wide
    tables) write what the CPU checker's object path writes -- each through its wide entry of the engine, once, and through no
    exact_count of a union inside the command's window --; `kij` through `dandd serve` writes the bytes of the one-shot."""
    from dandd_amd.engine import Engine
    from dandd_amd.host import deltatree
    seen = []                                                            # (entry, inputs) of every engine call that counts

    def counted(name):
        inner = getattr(Engine, name)

        def call(self, paths, *args, **kw):
            seen.append((name, len(paths), int(args[0])))          # (args[0]: k of exact_count, kmin of a table)
            return inner(self, paths, *args, **kw)
        monkeypatch.setattr(Engine, name, call)
    for name in ("exact_wide_pairwise", "exact_wide_progressive", "exact_wide_leave_out", "exact_count"):
        counted(name)
    gpu, chk = tmp_path / "gpu", tmp_path / "cpu"
    gpu.mkdir(), chk.mkdir()
    try:
        deltatree.set_backend_factory(None)
        pk, left_gpu = host_cpu.wide_tree(str(gpu), deltatree, backend=None)
        pkc, left_chk = host_cpu.wide_tree(str(chk), deltatree, backend=hostcheck.ExactBackend)
        for i, ((command, argv, _), (_, argv_chk, _)) in enumerate(zip(host_cpu.wide_commands(left_gpu), host_cpu.wide_commands(left_chk))):
            a, b = str(gpu / f"o{i}"), str(chk / f"o{i}")
            deltatree.set_backend_factory(None)
            del seen[:]
            cpu.run(deltatree, None, command, argv, pk, a)
            wide = ("exact_wide_pairwise", "exact_wide_progressive", "exact_wide_leave_out")[i]
            tables = [s for s in seen if s[0].startswith("exact_wide")]
            assert [s[:2] for s in tables] == [(wide, host_cpu.N_TREE)] and tables[0][2] <= 9, (command, tables)
            # no union of the command's window (--mink 9 --maxk 10) counted on its own; a climb that leaves the table may
            inside = [s for s in seen if s[0] == "exact_count" and s[1] >= 2 and 9 <= s[2] <= 10]
            assert not inside, (command, inside[:8])
            cpu.run(deltatree, hostcheck.ExactBackend, command, argv_chk, pkc, b, prefetch=False)
            names = sorted(os.path.basename(f) for f in os.listdir(a) if f.endswith(".csv"))
            assert names and names == sorted(os.path.basename(f) for f in os.listdir(b) if f.endswith(".csv"))
            for name in names:
                with open(os.path.join(a, name)) as x, open(os.path.join(b, name)) as y:
                    ta, tb = x.read(), y.read()
                if "command" in ta.splitlines()[0].split(","):
                    assert hostcheck.read_rows(os.path.join(a, name)) == hostcheck.read_rows(os.path.join(b, name)), (command, name)
                else:
                    assert ta.replace(str(gpu), "W") == tb.replace(str(chk), "W"), (command, name)
    finally:
        deltatree.set_backend_factory(None)
    # kij once more, in a process of its own and through the server
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = host_cpu.wide_commands(left_gpu)[0][1]
    one = str(tmp_path / "one")
    os.makedirs(one)
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "kij", "-d", pk, "-o", one, *argv], env=env, cwd=ROOT,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sock = os.path.join(sock_dir, "wd.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        os.makedirs(via)
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", "kij", "-d", pk, "-o", via, *argv], env=cenv,
                           cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        names = sorted(f for f in os.listdir(one) if f.endswith(".csv"))
        assert len(names) >= 2 and names == sorted(f for f in os.listdir(via) if f.endswith(".csv"))
        for name in names:
            with open(os.path.join(one, name), "rb") as x, open(os.path.join(via, name), "rb") as y, \
                    open(os.path.join(str(gpu / "o0"), name), "rb") as z:
                assert x.read() == y.read() == z.read(), name
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()


# ---- 10. size run -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_size_128_genomes_500kbp(engine_factory, torch_cuda, k):
    """128 x 500 kbp synthetic genomes (31 000 chunks of sorted k-mers, tens per workgroup: what the small cases above cannot
    show): device time (DD_KERNEL_EXACT) and wall time of every wide schedule next to one exact_count of all 128 buffers --
    printed, not asserted; ten unions of each schedule against exact_count_device of the corresponding buffers, and the
    number of distinct k-mers against exact_count_device of all."""
    from dandd_amd.engine import KERNEL_EXACT, synth_size
    eng = engine_factory()
    torch = torch_cuda
    n, nb = 128, 500_000
    bufs, sizes = [], []
    for gi in range(n):
        size = synth_size(nb, 4)
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(0xD4ADD, gi, nb, 4, t.data_ptr())
        bufs.append(t)
        sizes.append(size)
    eng.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    rng = np.random.default_rng(k)
    ords = [[int(x) for x in rng.permutation(n)] for _ in range(10)]
    group = [int(g) for g in rng.integers(-1, 10, n)]
    group[:10] = range(10)                                               # (every group has a member)

    def count(members):
        members = sorted(members)
        return eng.exact_count_device([ptrs[i] for i in members], [sizes[i] for i in members], k)

    calls = [("exact_count(all 128)", lambda: eng.exact_count_device(ptrs, sizes, k)),
             ("exact_wide_pairwise", lambda: eng.exact_wide_pairwise_device(ptrs, sizes, k, k)),
             ("exact_wide_leave_out (10 groups)", lambda: eng.exact_wide_leave_out_device(ptrs, sizes, k, k, group, 10)),
             ("exact_wide_progressive (10 orderings)", lambda: eng.exact_wide_progressive_device(ptrs, sizes, k, k, ords))]
    got = {}
    print()
    for name, call in calls:
        call()                                                  # (first launch, workspaces)
        eng.timing_enable(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        got[name] = call()
        wall = time.perf_counter() - t0
        ms, spans = eng.timing_read(KERNEL_EXACT)
        eng.timing_enable(False)
        print(f"128 x 500 kbp, k = {k}: {name}: {ms:.2f} ms device ({spans} spans), {wall * 1e3:.2f} ms call")
    M = got["exact_count(all 128)"]
    pw, lo, pr = (got[c[0]] for c in calls[1:])
    assert int(lo[10, 0]) == M and all(int(pr[o, n - 1, 0]) == M for o in range(10))
    for i, j in [(0, 0), (0, 127), (63, 64), (64, 64), (5, 70), (100, 127), (127, 127), (1, 65), (31, 96), (64, 127)]:
        assert int(pw[i, j, 0]) == int(pw[j, i, 0]) == count({i, j}), (i, j)
    for g in range(10):
        assert int(lo[g, 0]) == count([i for i in range(n) if group[i] != g]), g
    for o, j in [(0, 0), (1, 1), (2, 10), (3, 63), (4, 64), (5, 65), (6, 100), (7, 126), (8, 127), (9, 32)]:
        assert int(pr[o, j, 0]) == count(ords[o][:j + 1]), (o, j)
