"""dd_exact_pairwise / _progressive / _leave_out / _subsets on the MI355X: every union's count compared with == against the
oracle's exact counter (orc.exact_count of the union in question), single-pass and multi-pass, both ways a k-mer carries
its genome (key byte: k <= 28 and 33..60; byte array: 29..32 and 61..64), the all-ones run that unwritten slots share with a
genuine T^k, the device forms, the limits, the host layer end to end on a real `--exact` tree, and a size run (printed)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import hostcheck
import test_exact_schedules as cpu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [1, 2, 5, 11, 16, 21, 31, 32, 33, 48, 64]
RANGES = [(k, k) for k in KS] + [(2, 5), (30, 33), (61, 64)]          # 1 and 4 columns; both tag modes inside (30, 33)
NS = [1, 2, 3, 8, 33, 64]
LENGTH = {1: 4000, 2: 3000, 3: 2500, 8: 1500, 12: 400, 16: 400, 33: 400, 64: 200}


def genomes(n, length, seed):
    """Like the golden FASTAs: one ancestor, 3 % substitutions per genome, in several records, with an N run and a
    lowercase stretch.  From n = 3 on the last file is empty; from n = 8 on file 3 is file 1 byte for byte and file 4 is
    9 bases long (shorter than most k)."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length)
    out = []
    for i in range(n):
        s = anc.copy()
        mut = rng.random(length) < 0.03
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        t = "".join("ACGT"[c] for c in s)
        a, b = length // 3, 2 * length // 3
        t = t[:a] + "N" * (1 + i % 7) + t[a:b].lower() + t[b:]
        cut = [0, len(t) // 4 + i, len(t) // 2, len(t)]
        text = "".join(f">g{i}_r{r} record\n" + "\n".join(t[x:y][j:j + 70] for j in range(0, y - x, 70)) + "\n"
                       for r, (x, y) in enumerate(zip(cut, cut[1:])))
        out.append(text.encode())
    if n >= 3:
        out[n - 1] = b""
    if n >= 8:
        out[3] = out[1]
        out[4] = b">short\nACGTTGCAT\n"
    return out


def write(tmp_path, fas, tag="g"):
    paths = []
    for i, f in enumerate(fas):
        p = str(tmp_path / f"{tag}{i}.fa")
        with open(p, "wb") as fh:
            fh.write(f)
        paths.append(p)
    return paths


class Oracle:
    def __init__(self, orc, fas, canonical):
        self.orc, self.fas, self.canonical, self.memo = orc, fas, canonical, {}

    def __call__(self, members, k):
        key = (frozenset(int(i) for i in members), int(k))
        if not key[0]:
            return 0
        if key not in self.memo:
            self.memo[key] = self.orc.exact_count([self.fas[i] for i in sorted(key[0])], int(k), self.canonical)
        return self.memo[key]


def orderings(n, seed):
    rng = np.random.default_rng(seed)
    return [list(range(n)), list(range(n))[::-1]] + [[int(x) for x in rng.permutation(n)] for _ in range(5)]


def groupings(n):
    """singletons; two groups plus ungrouped leaves"""
    out = []
    if n >= 2:
        out.append(list(range(n)))
    if n >= 3:
        out.append([(0, 1, -1)[i % 3] if i < n - 1 else 1 for i in range(n)])
    return out


def masks_of(rng, n):
    """every mask for n <= 8; else the singletons, the full set, the complements of singletons and 64 seeded masks per size
    (the sampling of test_gpu_abba._masks)"""
    full = (1 << n) - 1
    if n <= 8:
        return list(range(1 << n))
    out = {full} | {1 << i for i in range(n)} | {full ^ (1 << i) for i in range(n)}
    for size in range(1, n + 1):
        for _ in range(64):
            out.add(int(sum(1 << int(i) for i in rng.choice(n, size=size, replace=False))))
    return sorted(out)


def check_all(eng, paths, want, n, kmin, kmax, seed, subsets_only=False):
    """every schedule over kmin..kmax against the oracle `want`; -> the arrays"""
    ks = list(range(kmin, kmax + 1))
    K = len(ks)
    M = [eng.exact_count(paths, k) for k in ks]
    assert M == [want(range(n), k) for k in ks]
    got = {}
    if not subsets_only:
        pw = got["pairwise"] = eng.exact_pairwise(paths, kmin, kmax)
        assert pw.shape == (n, n, K) and pw.dtype == np.uint64
        for i in range(n):
            for j in range(n):
                for kk, k in enumerate(ks):
                    assert int(pw[i, j, kk]) == want({i, j}, k), ("pairwise", n, k, i, j)
        ords = orderings(n, seed)
        pr = got["progressive"] = eng.exact_progressive(paths, kmin, kmax, ords)
        assert pr.shape == (len(ords), n, K)
        for o, order in enumerate(ords):
            for j in range(n):
                for kk, k in enumerate(ks):
                    assert int(pr[o, j, kk]) == want(order[:j + 1], k), ("progressive", n, k, o, j)
            assert [int(v) for v in pr[o, n - 1]] == M
        for gi, group in enumerate(groupings(n)):
            G = max(group) + 1
            lo = got[f"leave_out{gi}"] = eng.exact_leave_out(paths, kmin, kmax, group, G)
            assert lo.shape == (G + 1, K)
            for g in range(G):
                for kk, k in enumerate(ks):
                    assert int(lo[g, kk]) == want([i for i in range(n) if group[i] != g], k), ("leave_out", n, k, g)
            assert [int(v) for v in lo[G]] == M
    if n <= 16:
        sb = got["subsets"] = eng.exact_subsets(paths, kmin, kmax)
        assert sb.shape == (1 << n, K)
        assert not sb[0].any()
        for s in masks_of(np.random.default_rng(seed + 1), n):
            for kk, k in enumerate(ks):
                assert int(sb[s, kk]) == want([i for i in range(n) if s >> i & 1], k), ("subsets", n, k, s)
        assert [int(v) for v in sb[(1 << n) - 1]] == M
    return got


# ---- 1. every union against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_schedules_match_oracle(engine_factory, orc, tmp_path, n, canonical):
    eng = engine_factory(canonical=canonical)
    fas = genomes(n, LENGTH[n], 1000 + n)
    paths = write(tmp_path, fas)
    want = Oracle(orc, fas, canonical)
    for kmin, kmax in RANGES:
        check_all(eng, paths, want, n, kmin, kmax, seed=n)
        assert eng.last_sketch_stats()[2] == 1                   # (everything at once)


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", [12, 16])
def test_sampled_subsets_match_oracle(engine_factory, orc, tmp_path, n, canonical):
    eng = engine_factory(canonical=canonical)
    fas = genomes(n, LENGTH[n], 2000 + n)
    paths = write(tmp_path, fas)
    want = Oracle(orc, fas, canonical)
    for kmin, kmax in RANGES:
        check_all(eng, paths, want, n, kmin, kmax, seed=n, subsets_only=True)


def test_more_orderings_than_one_launch_holds(engine_factory, orc, tmp_path):
    """60 orderings of 64 genomes: the prefix masks and histograms of 53 fit the LDS of one launch, the rest go to a second
    launch over the same sorted k-mers (which must not count M again)."""
    n, canonical = 64, True
    eng = engine_factory(canonical=canonical)
    fas = genomes(n, LENGTH[n], 4000)
    paths = write(tmp_path, fas)
    want = Oracle(orc, fas, canonical)
    rng = np.random.default_rng(60)
    ords = [[int(x) for x in rng.permutation(n)] for _ in range(60)]
    for kmin, kmax in [(21, 21), (30, 33)]:
        ks = list(range(kmin, kmax + 1))
        pr = eng.exact_progressive(paths, kmin, kmax, ords)
        assert pr.shape == (60, n, len(ks))
        for o, order in enumerate(ords):
            for j in list(range(0, n, 7)) + [n - 2, n - 1]:
                assert [int(v) for v in pr[o, j]] == [want(order[:j + 1], k) for k in ks], (o, j)
        assert np.array_equal(pr[:7], eng.exact_progressive(paths, kmin, kmax, ords[:7]))
        assert np.array_equal(pr[50:], eng.exact_progressive(paths, kmin, kmax, ords[50:]))


def test_argument_rules(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    eng = engine_factory()
    paths = write(tmp_path, genomes(3, 500, 5))
    with pytest.raises(EngineError, match="holds every leaf"):
        eng.exact_leave_out(paths, 11, 11, [0, 0, 0], 1)
    with pytest.raises(EngineError, match="outside -1..0"):
        eng.exact_leave_out(paths, 11, 11, [0, 1, -1], 1)
    with pytest.raises(EngineError, match="not a permutation"):
        eng.exact_progressive(paths, 11, 11, [[0, 1, 1]])
    with pytest.raises(EngineError, match="outside 0..2"):
        eng.exact_progressive(paths, 11, 11, [[0, 1, 3]])
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_pairwise(paths, 0, 11)
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_pairwise(paths, 60, 65)
    with pytest.raises(EngineError):
        eng.exact_pairwise(paths[:2] + [str(tmp_path / "missing.fa")], 11, 11)


# ---- 2. passes over parts of the k-mer space -------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_multi_pass_gives_identical_arrays(engine_factory, orc, tmp_path, n, canonical):
    """The cases of test 1 on inputs of 320 kbp in all, with a 1 MiB budget: a pass holds whole bins of the k-mer space and at
    most max(65 536, largest bin) k-mers, so the 320 000 occurrences take at least three passes -- which dd_last_sketch_stats
    must report -- in every case but one: canonical k = 1 has two distinct k-mers, A and C, which are two bins and two passes
    whatever the budget and the inputs; there exactly those two are required.  The arrays equal the single-pass ones, and a
    handful of unions of every schedule the oracle's count on these inputs."""
    eng = engine_factory(canonical=canonical)
    fas = genomes(n, 320_000 // n + 200, 3000 + n)
    paths = write(tmp_path, fas)
    want = Oracle(orc, fas, canonical)
    groups = groupings(n)
    ords = orderings(n, n)

    def calls(kmin, kmax):
        yield "pairwise", lambda: eng.exact_pairwise(paths, kmin, kmax)
        yield "progressive", lambda: eng.exact_progressive(paths, kmin, kmax, ords)
        for group in groups:
            yield "leave_out", lambda group=group: eng.exact_leave_out(paths, kmin, kmax, group, max(group) + 1)
        if n <= 16:
            yield "subsets", lambda: eng.exact_subsets(paths, kmin, kmax)

    assert "DD_EXACT_MB" not in os.environ
    for kmin, kmax in RANGES:
        for what, call in calls(kmin, kmax):
            one = call()
            assert eng.last_sketch_stats()[2] == 1
            os.environ["DD_EXACT_MB"] = "1"
            try:
                many = call()
                passes = eng.last_sketch_stats()[2]
            finally:
                del os.environ["DD_EXACT_MB"]
            print(f"n={n} canonical={canonical} k={kmin}..{kmax} {what}: {passes} passes")
            if canonical and kmax == 1:
                assert passes == 2, (what, passes)
            else:
                assert passes >= 3, (what, kmin, kmax, passes)
            assert np.array_equal(one, many), (what, kmin, kmax)
            ks = range(kmin, kmax + 1)

            def same(row, members):
                assert [int(v) for v in row] == [want(members, k) for k in ks], (what, kmin, kmax, sorted(members))
            if what == "pairwise":
                for i, j in {(0, 0), (0, n - 1), (n // 2, n - 1), (min(1, n - 1), min(3, n - 1))}:
                    same(many[i, j], {i, j})
            if what == "progressive":
                for o, j in {(0, n - 1), (1, n // 2), (4, n // 3), (6, min(1, n - 1))}:
                    same(many[o, j], ords[o][:j + 1])
                assert [int(v) for v in many[0, n - 1]] == [eng.exact_count(paths, k) for k in ks]      # M
            if what == "leave_out":
                group = groups[0] if many.shape[0] == n + 1 else groups[-1]
                for g in {0, many.shape[0] - 2}:
                    same(many[g], [i for i in range(n) if group[i] != g])
                same(many[-1], range(n))
            if what == "subsets":
                full = (1 << n) - 1
                for m in {full, full ^ 1, 5 & full, 0xA6 & full} - {0}:
                    same(many[m], [i for i in range(n) if m >> i & 1])


# ---- 3. T^k and the slots nothing was written to ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 21, 31, 40, 63])
def test_all_t_kmer_shares_its_run_with_unwritten_slots(engine_factory, orc, tmp_path, k):
    """canonical = 0: T^k survives as the all-ones key, the value unwritten slots of the single-pass layout hold.  It is
    counted once, in exactly the unions that hold the genome with the T run."""
    eng = engine_factory(canonical=False)
    rng = np.random.default_rng(k)
    body = ["".join("ACGT"[c] for c in rng.integers(0, 4, 600)).replace("T" * 5, "TTGTT") for _ in range(3)]
    with_t = (">t\n" + body[0] + "T" * 100 + body[1] + "\n").encode()
    without = (">n\n" + body[0] + "N" + body[1] + "\n>m\n" + body[2] + "\n").encode()
    tk = (">q\n" + "T" * k + "\n").encode()
    assert orc.exact_count([without, tk], k, False) == orc.exact_count([without], k, False) + 1     # (T^k is not in `without`)
    assert orc.exact_count([with_t, tk], k, False) == orc.exact_count([with_t], k, False)          # (... and is in `with_t`)
    fas = [with_t, without, without]
    paths = write(tmp_path, fas)
    want = Oracle(orc, fas, False)
    got = check_all(eng, paths, want, 3, k, k, seed=k)
    assert eng.last_sketch_stats()[2] == 1
    sb = got["subsets"][:, 0]
    for s in range(1, 8):
        assert int(sb[s]) == orc.exact_count([fas[i] for i in range(3) if s >> i & 1] + ([tk] if s & 1 else []), k, False)
        if not s & 1:
            assert int(sb[s | 1]) > int(sb[s])


# ---- 4. device forms, limits -------------------------------------------------------------------------------------------
def test_device_forms_equal_path_forms(engine_factory, torch_cuda, tmp_path):
    eng = engine_factory()
    n = 8
    fas = genomes(n, 3000, 77)
    paths = write(tmp_path, fas)
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    ords, group = orderings(n, 3), groupings(n)[1]
    for kmin, kmax in [(5, 8), (21, 21), (30, 33), (61, 64)]:
        assert np.array_equal(eng.exact_pairwise_device(ptrs, sizes, kmin, kmax), eng.exact_pairwise(paths, kmin, kmax))
        assert np.array_equal(eng.exact_progressive_device(ptrs, sizes, kmin, kmax, ords), eng.exact_progressive(paths, kmin, kmax, ords))
        assert np.array_equal(eng.exact_leave_out_device(ptrs, sizes, kmin, kmax, group), eng.exact_leave_out(paths, kmin, kmax, group))
        assert np.array_equal(eng.exact_subsets_device(ptrs, sizes, kmin, kmax), eng.exact_subsets(paths, kmin, kmax))


def test_limits(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    one = write(tmp_path, genomes(1, 300, 9))
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_pairwise(one * 65, 11, 11)
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_progressive(one * 65, 11, 11, [list(range(65))])
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_leave_out(one * 65, 11, 11, list(range(65)))
    with pytest.raises(EngineError, match="outside 1..16"):
        eng.exact_subsets(one * 17, 11, 11)
    with pytest.raises(EngineError, match="outside 1..64"):
        eng.exact_pairwise([], 11, 11)
    be = HipExactBackend()
    try:
        rows = [[f"leaf{i}.k11"] for i in range(65)]
        assert be.pairwise_cards(rows) is None
        assert be.progressive_cards(rows, [list(range(65))]) is None
        assert be.leave_out_cards(rows, list(range(65))) is None
        assert be.subset_cards(rows[:17]) is None
    finally:
        be.close()


# ---- 5. the host layer end to end --------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, sock_dir, torch_cuda):
    """The five commands on a real `--exact` tree (HipExactBackend) write what the CPU checker writes -- row for row, byte for
    byte where a file has no `command` column -- and ref_exact.json's numbers; `kij` through `dandd serve` + the client writes
    the same bytes."""
    from dandd_amd.host import deltatree
    gpu, chk = tmp_path / "gpu", tmp_path / "cpu"
    gpu.mkdir(), chk.mkdir()
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(gpu), deltatree, backend=None)
        pkc = cpu.exact_tree(str(chk), deltatree, backend=cpu.ExactSchedules)
        for i, (command, argv, _) in enumerate(cpu.COMMANDS):
            a, b = str(gpu / f"o{i}"), str(chk / f"o{i}")
            deltatree.set_backend_factory(None)
            cpu.run(deltatree, None, command, argv, pk, a)
            cpu.run(deltatree, cpu.ExactSchedules, command, argv, pkc, b)
            names = sorted(os.path.basename(f) for f in os.listdir(a) if f.endswith(".csv"))
            assert names and names == sorted(os.path.basename(f) for f in os.listdir(b) if f.endswith(".csv"))
            for name in names:
                with open(os.path.join(a, name)) as x, open(os.path.join(b, name)) as y:
                    ta, tb = x.read(), y.read()
                if "command" in ta.splitlines()[0].split(","):
                    assert hostcheck.read_rows(os.path.join(a, name)) == hostcheck.read_rows(os.path.join(b, name)), (command, name)
                else:
                    assert ta.replace(str(gpu), "W") == tb.replace(str(chk), "W"), (command, name)
            if command in ("kij", "progressive"):
                cpu.against_goldens(command, a)
    finally:
        deltatree.set_backend_factory(None)
    # kij once more, in a process of its own and through the server
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = cpu.COMMANDS[0][1]
    one = str(tmp_path / "one")
    os.makedirs(one)
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "kij", "-d", pk, "-o", one, *argv], env=env, cwd=ROOT,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sock = os.path.join(sock_dir, "ex.sock")
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
        for name in ("gold_5_kmc.kij.csv", "gold_5_kmc.j.csv"):
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


# ---- 6. size run ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31, 40, 63])
def test_size_16_genomes_5mbp(engine_factory, torch_cuda, k):
    """16 x 5 Mbp synthetic genomes (39 000 chunks of sorted k-mers, 38 per workgroup: what the small cases above cannot
    show), one k per way of carrying the genome: device time (DD_KERNEL_EXACT) and wall time of every schedule next to one
    exact_count of all 16 buffers -- printed, not asserted; ten results against exact_count_device of the corresponding
    unions, and every pair, prefix and complement against the same union in the table of all subsets."""
    from dandd_amd.engine import KERNEL_EXACT, synth_size
    eng = engine_factory()
    torch = torch_cuda
    n, nb = 16, 5_000_000
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

    def count(members):
        members = sorted(members)
        return eng.exact_count_device([ptrs[i] for i in members], [sizes[i] for i in members], k)

    calls = [("exact_count(all 16)", lambda: eng.exact_count_device(ptrs, sizes, k)),
             ("exact_pairwise", lambda: eng.exact_pairwise_device(ptrs, sizes, k, k)),
             ("exact_subsets", lambda: eng.exact_subsets_device(ptrs, sizes, k, k)),
             ("exact_leave_out (singletons)", lambda: eng.exact_leave_out_device(ptrs, sizes, k, k, list(range(n)))),
             ("exact_progressive (10 orderings)", lambda: eng.exact_progressive_device(ptrs, sizes, k, k, ords))]
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
        print(f"16 x 5 Mbp, k = {k}: {name}: {ms:.2f} ms device ({spans} spans), {wall * 1e3:.2f} ms call")
    M = got["exact_count(all 16)"]
    pw, sb, lo, pr = (got[c[0]] for c in calls[1:])
    assert int(sb[-1, 0]) == int(lo[n, 0]) == int(pr[0, n - 1, 0]) == M
    assert int(pw[2, 11, 0]) == count({2, 11}) and int(pw[7, 7, 0]) == count({7})
    for s in (0x0003, 0x8001, 0x0F0F, 0x7FFF):
        assert int(sb[s, 0]) == count([i for i in range(n) if s >> i & 1]), hex(s)
    assert int(lo[5, 0]) == count(set(range(n)) - {5}) and int(lo[0, 0]) == int(sb[0xFFFE, 0])
    assert int(pr[3, 6, 0]) == count(ords[3][:7]) and int(pr[9, 0, 0]) == count(ords[9][:1])
    full = (1 << n) - 1
    assert [int(v) for v in lo[:n, 0]] == [int(sb[full ^ (1 << g), 0]) for g in range(n)]
    assert [[int(v) for v in row] for row in pw[:, :, 0]] == [[int(sb[(1 << i) | (1 << j), 0]) for j in range(n)] for i in range(n)]
    for o, order in enumerate(ords):
        assert [int(v) for v in pr[o, :, 0]] == [int(sb[sum(1 << g for g in order[:j + 1]), 0]) for j in range(n)]
    two = eng.exact_leave_out_device(ptrs, sizes, k, k, [0] * 8 + [1] * 7 + [-1])
    assert [int(v) for v in two[:, 0]] == [int(sb[0xFF00, 0]), int(sb[0x80FF, 0]), M]
