"""dd_exact_spectrum / _core_progressive / _select on the MI355X: every entry compared with == against membership masks built
in Python from pyref.kmers, at both key widths and both ways a k-mer carries its genome, single-pass and multi-pass, the
device forms, the argument rules, the identities that tie the three tables to the union schedules, the host layer end to
end on a real `--exact` tree, and a size run (tens of chunks per workgroup, which no small case reaches)."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import hostcheck
import pyref
import test_core as cpuc
import test_exact_schedules as cpu
import test_gpu_exact_schedules as sched

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KS = [1, 5, 21, 31, 33, 48, 62]
RANGES = [(k, k) for k in KS] + [(30, 33)]                    # both tag modes inside (30, 33)
NS = sched.NS
U64 = (1 << 64) - 1


def masks_array(fas, k, canonical):
    """the membership masks of the distinct k-mers of FASTA buffers `fas`, from pyref.kmers: uint64 [M]"""
    return np.array(list(cpuc.masks_of(fas, k, canonical).values()), dtype=np.uint64)


def want_spectrum(m, n):
    pc = np.array([bin(int(x)).count("1") for x in m], dtype=np.int64)
    return [int((pc == j).sum()) for j in range(n + 1)]


def want_select(m, al, no):
    al, no = np.uint64(al), np.uint64(no)
    return int((((m & al) == al) & ((m & no) == np.uint64(0))).sum())


def want_core(m, order):
    out, need = [], 0
    for g in order:
        need |= 1 << g
        out.append(want_select(m, need, 0))
    return out


def queries(n, seed):
    """every singleton, every pair, the full set, (0, 0), each (G, full ^ G) of the groupings, and 200 seeded random
    (all, none): disjoint ones, overlapping ones (which count 0) and empty sides"""
    full = (1 << n) - 1
    qs = [(1 << i, 0) for i in range(n)] + [(1 << i | 1 << j, 0) for i in range(n) for j in range(i + 1, n)] + [(full, 0), (0, 0)]
    for group in sched.groupings(n):
        for g in range(max(group) + 1):
            G = sum(1 << i for i in range(n) if group[i] == g)
            qs.append((G, full ^ G))
    rng = np.random.default_rng(seed)
    for r in range(200):
        a = int(sum(1 << int(i) for i in rng.choice(n, size=int(rng.integers(0, min(n, 4) + 1)), replace=False)))
        b = int(sum(1 << int(i) for i in rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False)))
        if r % 4:
            b &= ~a                                              # (three in four disjoint; the rest may overlap)
        qs.append((a, b))
    return qs


def check_tables(eng, paths, fas, n, canonical, kmin, kmax, seed):
    """the three tables over kmin..kmax against the masks; -> (spectrum, core, select, orderings, queries)"""
    ks = list(range(kmin, kmax + 1))
    ref = [masks_array(fas, k, canonical) for k in ks]
    spec = eng.exact_spectrum(paths, kmin, kmax)
    assert spec.shape == (n + 1, len(ks)) and spec.dtype == np.uint64
    for kk, m in enumerate(ref):
        assert [int(v) for v in spec[:, kk]] == want_spectrum(m, n), ("spectrum", n, ks[kk])
    ords = sched.orderings(n, seed)
    core = eng.exact_core_progressive(paths, kmin, kmax, ords)
    assert core.shape == (len(ords), n, len(ks)) and core.dtype == np.uint64
    for o, order in enumerate(ords):
        for kk, m in enumerate(ref):
            assert [int(v) for v in core[o, :, kk]] == want_core(m, order), ("core", n, ks[kk], o)
    qs = queries(n, seed)
    sel = eng.exact_select(paths, kmin, kmax, [a for a, _ in qs], [b for _, b in qs])
    assert sel.shape == (len(qs), len(ks)) and sel.dtype == np.uint64
    for kk, m in enumerate(ref):
        for q, (a, b) in enumerate(qs):
            assert int(sel[q, kk]) == want_select(m, a, b), ("select", n, ks[kk], hex(a), hex(b))
    return spec, core, sel, ords, qs


def check_identities(eng, paths, n, kmin, kmax, spec, core, sel, ords, qs):
    """what ties the three tables to dd_exact_count and the union schedules, same inputs"""
    ks = list(range(kmin, kmax + 1))
    M = [eng.exact_count(paths, k) for k in ks]
    own = [[eng.exact_count([p], k) for k in ks] for p in paths]
    at = {q: i for i, q in enumerate(qs)}
    full = (1 << n) - 1
    pr = eng.exact_progressive(paths, kmin, kmax, ords)
    pw = eng.exact_pairwise(paths, kmin, kmax)
    sb = eng.exact_subsets(paths, kmin, kmax) if n <= 16 else None
    for kk in range(len(ks)):
        assert sum(int(v) for v in spec[:, kk]) == M[kk]
        assert int(spec[0, kk]) == 0
        assert sum(j * int(spec[j, kk]) for j in range(n + 1)) == sum(own[i][kk] for i in range(n))
        assert int(sel[at[(0, 0)], kk]) == M[kk] and int(sel[at[(full, 0)], kk]) == int(spec[n, kk])
        for o in range(len(ords)):
            assert int(core[o, n - 1, kk]) == int(spec[n, kk])
            assert int(core[o, 0, kk]) == int(pr[o, 0, kk])
        for i in range(n):
            assert int(sel[at[(1 << i, 0)], kk]) == own[i][kk]
            for j in range(i + 1, n):
                assert int(sel[at[(1 << i | 1 << j, 0)], kk]) == own[i][kk] + own[j][kk] - int(pw[i, j, kk]), (i, j)
        if sb is not None:
            for a, b in qs:
                if a == 0:
                    assert int(sel[at[(a, b)], kk]) == M[kk] - int(sb[b, kk]), hex(b)


# ---- 1. every entry against the masks, and the identities ---------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_tables_match_masks(engine_factory, tmp_path, n, canonical):
    eng = engine_factory(canonical=canonical)
    fas = sched.genomes(n, sched.LENGTH[n], 1000 + n)
    paths = sched.write(tmp_path, fas)
    for kmin, kmax in RANGES:
        got = check_tables(eng, paths, fas, n, canonical, kmin, kmax, seed=n)
        assert eng.last_sketch_stats()[2] == 1                   # (everything at once)
        check_identities(eng, paths, n, kmin, kmax, *got)
    if n == 64:
        assert len(queries(n, n)) > 1024                         # (more queries than one select launch holds)


def test_full_mask_of_64_genomes(engine_factory, tmp_path):
    """64 non-empty genomes that share their middle 80 bases: bin 64 of the spectrum, select(~0, 0) and the last step of
    every core are non-zero -- the family above ends in an empty file and never sets bit 63 of a full mask."""
    n, length, canonical = 64, 200, True
    eng = engine_factory(canonical=canonical)
    rng = np.random.default_rng(6464)
    anc = rng.integers(0, 4, length)
    fas = []
    for i in range(n):
        s = anc.copy()
        mut = rng.random(length) < 0.05
        mut[60:140] = False
        s[mut] = (s[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
        fas.append((f">f{i}\n" + "".join("ACGT"[c] for c in s) + "\n").encode())
    paths = sched.write(tmp_path, fas, tag="f")
    ords = sched.orderings(n, 64)
    for k in (5, 21, 33):
        m = masks_array(fas, k, canonical)
        spec = eng.exact_spectrum(paths, k, k)
        assert [int(v) for v in spec[:, 0]] == want_spectrum(m, n)
        assert int(spec[64, 0]) > 0
        sel = eng.exact_select(paths, k, k, [U64, U64, 0, 1 << 63], [0, 1, U64, 0])
        assert [int(v) for v in sel[:, 0]] == [want_select(m, U64, 0), 0, 0, want_select(m, 1 << 63, 0)]
        assert int(sel[0, 0]) == int(spec[64, 0])
        core = eng.exact_core_progressive(paths, k, k, ords)
        for o, order in enumerate(ords):
            assert [int(v) for v in core[o, :, 0]] == want_core(m, order), (k, o)
            assert int(core[o, 63, 0]) == int(spec[64, 0])


# ---- 2. passes over parts of the k-mer space -------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", NS)
def test_multi_pass_gives_identical_arrays(engine_factory, tmp_path, n, canonical):
    """320 kbp in all with a 1 MiB budget (the inputs of test_gpu_exact_schedules' multi-pass test): at least three passes,
    the same arrays as one pass, and rows that add up to dd_exact_count."""
    eng = engine_factory(canonical=canonical)
    fas = sched.genomes(n, 320_000 // n + 200, 3000 + n)
    paths = sched.write(tmp_path, fas)
    ords = sched.orderings(n, n)
    qs = queries(n, n)
    calls = [("spectrum", lambda a, b: eng.exact_spectrum(paths, a, b)),
             ("core_progressive", lambda a, b: eng.exact_core_progressive(paths, a, b, ords)),
             ("select", lambda a, b: eng.exact_select(paths, a, b, [q[0] for q in qs], [q[1] for q in qs]))]
    assert "DD_EXACT_MB" not in os.environ
    for kmin, kmax in [(5, 5), (21, 21), (30, 33), (48, 48)]:
        for what, call in calls:
            one = call(kmin, kmax)
            assert eng.last_sketch_stats()[2] == 1
            os.environ["DD_EXACT_MB"] = "1"
            try:
                many = call(kmin, kmax)
                passes = eng.last_sketch_stats()[2]
            finally:
                del os.environ["DD_EXACT_MB"]
            assert passes >= 3, (what, kmin, kmax, passes)
            assert np.array_equal(one, many), (what, kmin, kmax)
            if what == "spectrum":
                assert [int(v) for v in many.sum(axis=0)] == [eng.exact_count(paths, k) for k in range(kmin, kmax + 1)]


# ---- 3. device forms, argument rules -----------------------------------------------------------------------------------
def test_device_forms_equal_path_forms(engine_factory, torch_cuda, tmp_path):
    eng = engine_factory()
    n = 8
    fas = sched.genomes(n, 3000, 77)
    paths = sched.write(tmp_path, fas)
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    ords, qs = sched.orderings(n, 3), queries(n, 3)
    al, no = [q[0] for q in qs], [q[1] for q in qs]
    for kmin, kmax in [(5, 8), (21, 21), (30, 33), (61, 64)]:
        assert np.array_equal(eng.exact_spectrum_device(ptrs, sizes, kmin, kmax), eng.exact_spectrum(paths, kmin, kmax))
        assert np.array_equal(eng.exact_core_progressive_device(ptrs, sizes, kmin, kmax, ords), eng.exact_core_progressive(paths, kmin, kmax, ords))
        assert np.array_equal(eng.exact_select_device(ptrs, sizes, kmin, kmax, al, no), eng.exact_select(paths, kmin, kmax, al, no))


def test_argument_rules(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    from dandd_amd.host.backend import HipExactBackend
    eng = engine_factory()
    paths = sched.write(tmp_path, sched.genomes(3, 500, 5))
    one = paths[:1]
    for call in (lambda p, a, b: eng.exact_spectrum(p, a, b), lambda p, a, b: eng.exact_core_progressive(p, a, b, [list(range(len(p)))]),
                 lambda p, a, b: eng.exact_select(p, a, b, [1], [0])):
        with pytest.raises(EngineError, match="outside 1..64"):
            call([], 11, 11)                                      # n = 0
        with pytest.raises(EngineError, match="outside 1..64"):
            call(one * 65, 11, 11)                                # n = 65
        with pytest.raises(EngineError, match="outside 1..64"):
            call(paths, 0, 11)                                    # k = 0
        with pytest.raises(EngineError, match="outside 1..64"):
            call(paths, 60, 65)                                   # k = 65
        with pytest.raises(EngineError):
            call(paths[:2] + [str(tmp_path / "missing.fa")], 11, 11)
    with pytest.raises(EngineError, match="not a permutation"):
        eng.exact_core_progressive(paths, 11, 11, [[0, 1, 1]])
    with pytest.raises(EngineError, match="outside 0..2"):
        eng.exact_core_progressive(paths, 11, 11, [[0, 1, 3]])
    with pytest.raises(EngineError, match="outside 0..2"):
        eng.exact_select(paths, 11, 11, [8], [0])                 # bit 3 of `all`, n = 3
    with pytest.raises(EngineError, match="outside 0..2"):
        eng.exact_select(paths, 11, 11, [1, 2], [0, 1 << 63])     # bit 63 of `none`
    with pytest.raises(EngineError, match="at least one query"):
        eng.exact_select(paths, 11, 11, [], [])                   # nq = 0
    assert [int(v) for v in eng.exact_select(paths, 11, 11, [3], [1])[:, 0]] == [0]    # all & none != 0: legal, counts 0
    # null pointers, straight at the C ABI
    lib = eng._lib
    arr = (ctypes.c_char_p * 3)(*[os.fsencode(p) for p in paths])
    out = np.zeros(64, dtype=np.uint64)
    masks = np.zeros(1, dtype=np.uint64)
    for rc in (lib.dd_exact_spectrum(eng._ctx, arr, 3, 11, 11, None),
               lib.dd_exact_spectrum(eng._ctx, None, 3, 11, 11, out.ctypes.data),
               lib.dd_exact_core_progressive(eng._ctx, arr, 3, 11, 11, None, 1, out.ctypes.data),
               lib.dd_exact_select(eng._ctx, arr, 3, 11, 11, None, masks.ctypes.data, 1, out.ctypes.data),
               lib.dd_exact_select(eng._ctx, arr, 3, 11, 11, masks.ctypes.data, None, 1, out.ctypes.data),
               lib.dd_exact_select(eng._ctx, arr, 3, 11, 11, masks.ctypes.data, masks.ctypes.data, 1, None)):
        assert rc != 0 and ("null" in lib.dd_last_error().decode() or "bad argument" in lib.dd_last_error().decode())
    be = HipExactBackend()
    try:
        rows = [[f"leaf{i}.k11"] for i in range(65)]
        assert be.spectrum_counts(rows) is None
        assert be.core_progressive_counts(rows, [list(range(65))]) is None
        assert be.select_counts(rows, [1], [0]) is None
    finally:
        be.close()


# ---- 4. the host layer end to end ----------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, sock_dir, torch_cuda):
    """`core` on a real `--exact` tree (HipExactBackend) writes byte for byte what the CPU checker writes, one-shot and
    through `dandd serve` + the client."""
    from dandd_amd.host import deltatree
    gpu, chk = tmp_path / "gpu", tmp_path / "cpu"
    gpu.mkdir(), chk.mkdir()

    def files(d, root):
        out = cpuc._outputs(d)
        return {name: text.replace(str(root).encode(), b"W") for name, text in out.items()}

    def argv_for(root):
        groups = root / "groups.tsv"
        groups.write_text(f"{root / 'data' / 'g0.fasta'}\tleft\ng3.fasta\tright\ng2.fasta\tleft\ng4.fasta\tright\ng1.fasta\talone\n")
        return ["-r", str(root / "t" / "sketchdb" / "gold_5_orderings.pickle"), "-g", str(groups), *cpuc.WINDOW]
    try:
        deltatree.set_backend_factory(None)
        pk = cpu.exact_tree(str(gpu), deltatree, backend=None)
        pkc = cpu.exact_tree(str(chk), deltatree, backend=cpuc.CoreBackend)
        a, b = str(gpu / "o"), str(chk / "o")
        deltatree.set_backend_factory(None)
        cpu.run(deltatree, None, "core", argv_for(gpu), pk, a)
        cpu.run(deltatree, cpuc.CoreBackend, "core", argv_for(chk), pkc, b)
        got, want = files(a, gpu), files(b, chk)
        assert len(want) == 5 and got == want
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
    sock = os.path.join(sock_dir, "core.sock")
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


# ---- 5. size run ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 33])
def test_size_16_genomes_5mbp(engine_factory, torch_cuda, k):
    """16 x 5 Mbp synthetic genomes (39 000 chunks of sorted k-mers, 38 per workgroup -- the size at which the aggregation
    loop of DESIGN.md section 8 lost counts), one k per key width: the identities against the union schedules, the full core
    against inclusion-exclusion over all 65 535 rows of dd_exact_subsets, ten orderings' core[o][1] against dd_exact_pairwise;
    the wall time of every new call is printed."""
    from dandd_amd.engine import synth_size
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
    full = (1 << n) - 1
    pairs = [(1 << i | 1 << j, 0) for i in range(n) for j in range(i + 1, n)]
    nones = [(0, int(g)) for g in rng.integers(1, full, size=64)]
    many = pairs + nones + [(int(a), int(b) & ~int(a)) for a, b in zip(rng.integers(0, full + 1, size=1024), rng.integers(0, full + 1, size=1024))]
    many = many[:1024]
    calls = [("exact_spectrum", lambda: eng.exact_spectrum_device(ptrs, sizes, k, k)),
             ("exact_core_progressive (10 orderings)", lambda: eng.exact_core_progressive_device(ptrs, sizes, k, k, ords)),
             ("exact_select (nq = 1)", lambda: eng.exact_select_device(ptrs, sizes, k, k, [full], [0])),
             ("exact_select (nq = 64)", lambda: eng.exact_select_device(ptrs, sizes, k, k, [0] * 64, [q[1] for q in nones])),
             ("exact_select (nq = 1024)", lambda: eng.exact_select_device(ptrs, sizes, k, k, [q[0] for q in many], [q[1] for q in many]))]
    got = {}
    print()
    for name, call in calls:
        call()                                                  # (first launch, workspaces)
        t0 = time.perf_counter()
        got[name] = call()
        print(f"16 x 5 Mbp, k = {k}: {name}: {(time.perf_counter() - t0) * 1e3:.2f} ms call")
    spec, core, sel1, sel64, selmany = (got[c[0]][..., 0] for c in calls)
    M = eng.exact_count_device(ptrs, sizes, k)
    own = [eng.exact_count_device([ptrs[i]], [sizes[i]], k) for i in range(n)]
    pw = eng.exact_pairwise_device(ptrs, sizes, k, k)[..., 0]
    sb = eng.exact_subsets_device(ptrs, sizes, k, k)[..., 0]
    pr = eng.exact_progressive_device(ptrs, sizes, k, k, ords)[..., 0]
    assert sum(int(v) for v in spec) == M and int(spec[0]) == 0
    assert sum(j * int(spec[j]) for j in range(n + 1)) == sum(own)
    incl_excl = sum((-1) ** (bin(s).count("1") + 1) * int(sb[s]) for s in range(1, full + 1))
    assert int(spec[n]) == incl_excl == int(sel1[0])
    for o, order in enumerate(ords):
        assert int(core[o, n - 1]) == int(spec[n])
        assert int(core[o, 0]) == int(pr[o, 0]) == own[order[0]]
        a, b = order[0], order[1]
        assert int(core[o, 1]) == own[a] + own[b] - int(pw[a, b])
        assert all(int(core[o, j]) >= int(core[o, j + 1]) for j in range(n - 1))
    assert [int(v) for v in sel64] == [M - int(sb[g]) for _, g in nones]
    for q, (a, b) in enumerate(many):
        if q < len(pairs):
            i, j = [x for x in range(n) if a >> x & 1]
            assert int(selmany[q]) == own[i] + own[j] - int(pw[i, j]), (i, j)
        elif a == 0:
            assert int(selmany[q]) == M - int(sb[b]), hex(b)
