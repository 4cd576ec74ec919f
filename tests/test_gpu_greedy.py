"""dd_extend / dd_greedy on the MI355X: "base U leaf_g" for every candidate from one read of the candidates' rows
(dd_extend.hip) against the oracle's card of the oracle's union -- doubles compared with == --, against dd_progressive's
prefixes, the greedy walk against a Python walk of the selection rule over oracle cards, the argument rules, the backend and
CLI paths (`dandd greedy`) against the CPU checker and `dandd serve`, and the 64-genome size with its time against the walk
emulated with dd_progressive."""
import glob
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import hostcheck

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _leaf(rng, n, K, p):
    return np.minimum(rng.geometric(0.5, size=(n, K, 1 << p)), 64 - p + 1).astype(np.uint8)


def _cards(orc, base, leaf, p):
    """want[g][kk] = orc.card(orc.union(base[kk], leaf[g][kk])); base None: the leaf's own card"""
    n, K, _ = leaf.shape
    out = np.empty((n, K))
    for g in range(n):
        for kk in range(K):
            out[g, kk] = orc.card(leaf[g, kk] if base is None else orc.union(base[kk], leaf[g, kk]), p)
    return out


# every n of {1, 2, 5, 17, 64, 70, 257, 300}, log2m of {4, 10, 14, 16, 17, 20} and K of {1, 3, 37} at least once; the large n
# with the small log2m and K (the largest slab here is 70 MiB)
CASES = [(1, 1, 4), (2, 3, 10), (5, 37, 14), (17, 3, 16), (64, 3, 17), (70, 1, 20), (257, 3, 10), (300, 37, 4), (300, 1, 14),
         (64, 37, 10), (2, 1, 20), (5, 3, 17)]


@pytest.mark.parametrize("n,K,p", CASES)
def test_extend_matches_oracle(engine_factory, torch_cuda, orc, n, K, p):
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(n * 1000 + K * 10 + p)
    leaf = _leaf(rng, n, K, p)
    dev = torch_cuda.from_numpy(leaf).cuda()
    subset = rng.permutation(n)[: max(1, n // 2)]
    repeat = np.concatenate([subset, subset[:1], [n - 1, n - 1]])
    bases = {"none": None, "a leaf": leaf[n // 2].copy(), "union of all": leaf.max(axis=0), "zeros": np.zeros_like(leaf[0])}
    for name, base in bases.items():
        want = _cards(orc, base, leaf, p)
        bdev = None if base is None else torch_cuda.from_numpy(base).cuda()
        bptr = 0 if base is None else bdev.data_ptr()
        assert np.array_equal(eng.extend_device(bptr, dev.data_ptr(), n, K), want), (name, "all rows")
        assert np.array_equal(eng.extend_device(bptr, dev.data_ptr(), n, K, subset), want[subset]), (name, "subset")
        assert np.array_equal(eng.extend_device(bptr, dev.data_ptr(), n, K, repeat), want[repeat]), (name, "repeat")
        assert np.array_equal(eng.extend(base, leaf, repeat), want[repeat]), (name, "host pointers")
        if name == "union of all":                        # no correction anywhere: every row is the base's own card
            assert (want == want[0]).all()
        if name == "zeros":
            assert np.array_equal(want, _cards(orc, None, leaf, p))


@pytest.mark.parametrize("n,K,p", [(9, 4, 14), (7, 2, 18), (40, 2, 12)])
def test_extend_equals_progressive_prefixes(engine_factory, torch_cuda, n, K, p):
    """dd_extend_device(base = union of ord[:j]) row g == dd_progressive_device's prefix j + 1 of the ordering (ord[:j], g,
    rest): the same integers, so the same doubles (log2m 18, n <= 32: the bit-plane scan; else the streaming kernel).  This
    is the walk as the schedules before dd_extend can run it."""
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(77 + n)
    leaf = _leaf(rng, n, K, p)
    dev = torch_cuda.from_numpy(leaf).cuda()
    order = [int(i) for i in rng.permutation(n)]
    for j in range(n):
        rest = order[j:]
        ords = [order[:j] + [g] + [x for x in rest if x != g] for g in rest]
        prog = eng.progressive_device(dev.data_ptr(), n, K, ords)[:, j, :]
        base = dev[order[j - 1]].clone() if j == 1 else (torch_cuda.maximum(base, dev[order[j - 1]]) if j else None)
        got = eng.extend_device(base.data_ptr() if j else 0, dev.data_ptr(), n, K, rest)
        assert np.array_equal(got, prog), j


def _delta(cards, ks):
    best = 0
    for c, k in zip(cards, ks):
        if c / k >= best:
            best = c / k
    return best


def _oracle_walk(orc, leaf, p, kmin, mode, cand, nfixed, nsteps):
    """the selection rule over oracle cards: cand[:nfixed] given, then the best remaining candidate, the earlier one of cand
    winning a tie"""
    K = leaf.shape[1]
    ks = list(range(kmin, kmin + K))
    order, cards, left, base = [], [], list(cand[nfixed:]), None
    for j in range(nsteps):
        rows = [cand[j]] if j < nfixed else left
        got = [[orc.card(leaf[c, kk] if base is None else orc.union(base[kk], leaf[c, kk]), p) for kk in range(K)] for c in rows]
        ds = [_delta(g, ks) for g in got]
        pick = 0
        for r in range(1, len(rows)):
            if (ds[r] > ds[pick]) if mode == 0 else (ds[r] < ds[pick]):
                pick = r
        c = rows[pick]
        order.append(c)
        cards.append(got[pick])
        if j >= nfixed:
            left.pop(pick)
        base = leaf[c].copy() if base is None else np.maximum(base, leaf[c])
    return np.array(order, dtype=np.int32), np.array(cards)


GREEDY_SEED = 512      # (one default_rng stream for every draw, as the seeded sweeps of tests/test_gpu_fuzz.py)


def test_greedy_matches_oracle_walk(engine_factory, torch_cuda, orc):
    rng = np.random.default_rng(GREEDY_SEED)
    for n, K, p, kmin in [(12, 5, 12, 8), (6, 3, 16, 30), (20, 2, 10, 1), (3, 1, 4, 64)]:
        eng = engine_factory(log2m=p)
        leaf = _leaf(rng, n, K, p)
        leaf[1] = np.minimum(leaf[1], 2)            # a small genome and a large one: the two modes part at once
        leaf[n - 1] = np.maximum(leaf[n - 1], 3)
        dev = torch_cuda.from_numpy(leaf).cuda()
        everyone = list(range(n))
        some = [int(i) for i in rng.permutation(n)[: max(2, n - 3)]]                    # a strict subset, shuffled
        for mode in (0, 1):
            for cand, nfixed, nsteps in [(everyone, 0, n), (everyone, 1, n), (everyone, min(3, n), n), (everyone, 0, max(1, n // 2)),
                                         (some, 0, len(some)), (some, 1, len(some) - 1), (some, min(3, len(some)), min(3, len(some)))]:
                order, cards = eng.greedy_device(dev.data_ptr(), n, K, kmin, mode, cand, nfixed, nsteps)
                worder, wcards = _oracle_walk(orc, leaf, p, kmin, mode, cand, nfixed, nsteps)
                assert np.array_equal(order, worder), (n, mode, cand, nfixed, nsteps)
                assert np.array_equal(cards, wcards), (n, mode, cand, nfixed, nsteps)
            horder, hcards = eng.greedy(leaf, kmin, mode, some, 1, len(some))
            dorder, dcards = eng.greedy_device(dev.data_ptr(), n, K, kmin, mode, some, 1, len(some))
            assert np.array_equal(horder, dorder) and np.array_equal(hcards, dcards)
        assert not np.array_equal(eng.greedy_device(dev.data_ptr(), n, K, kmin, 0)[0], eng.greedy_device(dev.data_ptr(), n, K, kmin, 1)[0])


def test_greedy_tie_goes_to_the_earlier_candidate(engine_factory, torch_cuda, orc):
    p, n, K, kmin = 12, 6, 4, 9
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(GREEDY_SEED + 1)
    leaf = _leaf(rng, n, K, p)
    leaf[4] = leaf[1]                                # leaf 4 is leaf 1 again
    dev = torch_cuda.from_numpy(leaf).cuda()
    swap = {1: 4, 4: 1}
    for mode in (0, 1):
        fwd = [0, 1, 2, 3, 4, 5]
        a, ca = eng.greedy_device(dev.data_ptr(), n, K, kmin, mode, fwd)
        b, cb = eng.greedy_device(dev.data_ptr(), n, K, kmin, mode, fwd[::-1])
        a, b = [int(x) for x in a], [int(x) for x in b]
        assert a.index(1) < a.index(4) and b.index(4) < b.index(1)
        assert b == [swap.get(x, x) for x in a] and np.array_equal(ca, cb)
        assert np.array_equal(a, _oracle_walk(orc, leaf, p, kmin, mode, fwd, 0, n)[0])
        assert np.array_equal(b, _oracle_walk(orc, leaf, p, kmin, mode, fwd[::-1], 0, n)[0])


def test_argument_rules(engine_factory, torch_cuda):
    from dandd_amd.engine import EngineError
    p, n, K = 10, 4, 3
    eng = engine_factory(log2m=p)
    leaf = np.ones((n, K, 1 << p), dtype=np.uint8)
    dev = torch_cuda.from_numpy(leaf).cuda()
    ptr = dev.data_ptr()
    with pytest.raises(EngineError, match="bad argument"):
        eng.extend_device(0, ptr, 0, K)
    with pytest.raises(EngineError, match="bad argument"):
        eng.extend_device(0, ptr, n, 0)
    with pytest.raises(EngineError, match="bad argument"):
        eng.extend_device(0, 0, n, K)
    with pytest.raises(EngineError, match="outside 0..3"):
        eng.extend_device(0, ptr, n, K, [0, 4])
    with pytest.raises(EngineError, match="outside 0..3"):
        eng.extend(None, leaf, [-1])
    with pytest.raises(EngineError, match="at least one row"):
        eng.extend_device(0, ptr, n, K, [])

    def greedy(kmin=5, mode=0, cand=(0, 1, 2, 3), nfixed=0, nsteps=None, n_=n, K_=K, leaf_ptr=ptr):
        return eng.greedy_device(leaf_ptr, n_, K_, kmin, mode, list(cand), nfixed, nsteps)
    for kw, text in [(dict(n_=0), "bad argument"), (dict(K_=0), "bad argument"), (dict(leaf_ptr=0), "bad argument"),
                     (dict(cand=(0, 4)), "outside 0..3"), (dict(cand=(0, -1)), "outside 0..3"), (dict(cand=(0, 1, 0)), "repeat"),
                     (dict(nfixed=3, nsteps=2), "nfixed=3"), (dict(nfixed=-1), "nfixed=-1"), (dict(nsteps=5), "nsteps=5"),
                     (dict(nsteps=0), "nsteps=0"), (dict(kmin=0), "k window"), (dict(kmin=63), "k window"), (dict(mode=2), "mode=2")]:
        with pytest.raises(EngineError, match=text):
            greedy(**kw)
    order, cards = greedy(kmin=62)                  # 62..64: the last window that fits
    assert sorted(order) == [0, 1, 2, 3] and cards.shape == (4, 3)


def _greedy_files(d):
    return {os.path.basename(f): open(f, "rb").read() for f in glob.glob(os.path.join(d, "*greedy*"))}


@pytest.mark.parametrize("regs", [14, 20])
def test_cli_end_to_end(tmp_path, regs, sock_dir, torch_cuda):
    """`greedy` with HipBackend writes the bytes the CPU checker writes; through `dandd serve` + the client the same again."""
    from dandd_amd.host import cli, deltatree
    import test_deltadelta as cpu
    import test_greedy as cpug
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    t = str(tmp_path / "g")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "tree", "-d", data, "-o", t, "-s", "gold", "-k", "10", "-r",
                    str(regs)], env=env, check=True, cwd=ROOT, timeout=300, capture_output=True)
    pk = os.path.join(t, "gold_5_dashing_dtree.pickle")
    basef = tmp_path / "base.txt"
    basef.write_text("g2.fasta\n")
    argv = ["greedy", "-d", pk, *cpug.WINDOW, "-b", str(basef)]
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", *argv, "-o", one], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the CPU checker: the same FASTA files (the rows name them by path), a tree and sketches of its own
    deltatree.set_backend_factory(lambda r_, c: hostcheck.OracleBackend(r_, c))
    try:
        _, pkc = cpu._tree(str(tmp_path), deltatree, registers=regs)
        deltatree.set_backend_factory(lambda r_, c: cpug.GreedyBackend(r_, c))
        cli.main(["greedy", "-d", pkc, *cpug.WINDOW, "-b", str(basef), "-o", str(tmp_path / "cpu")])
    finally:
        deltatree.set_backend_factory(None)
    got, want = _greedy_files(one), _greedy_files(str(tmp_path / "cpu"))
    assert len(want) == 4 and got == want
    sock = os.path.join(sock_dir, "dd.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        for _ in range(2):                            # (the second one over the slab the first left in HBM)
            r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", *argv, "-o", via], env=cenv,
                               cwd=ROOT, timeout=300, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert _greedy_files(via) == got
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()


def test_backend_reuses_the_slab_and_ties_follow_the_caller(torch_cuda, orc, tmp_path):
    """HipBackend.greedy_cards over leaves listed out of the slab's (sorted) order, two of them the same sketch: ties go to
    the leaf the caller lists first; a schedule after it finds the slab in HBM."""
    from dandd_amd.host.backend import HipBackend, write_sketch_file
    p, n, K, kmin = 14, 7, 4, 9
    rng = np.random.default_rng(GREEDY_SEED + 2)
    leaf = _leaf(rng, n, K, p)
    leaf[5] = leaf[2]
    be = HipBackend(log2m=p)
    try:
        paths = []
        for i in range(n):
            row = []
            for kk in range(K):
                path = str(tmp_path / f"leaf{(5 * i) % n}_{i}.k{kk + kmin}.hll")
                write_sketch_file(path, leaf[i, kk], p, kk + kmin, True)
                row.append(path)
            paths.append(row)
        assert sorted(range(n), key=lambda i: paths[i][0]) != list(range(n))
        uploads = []
        real = be.engine.device_upload
        be.engine.device_upload = lambda ptr, host: uploads.append(1) or real(ptr, host)
        for mode, code in (("max", 0), ("min", 1)):
            for listed in (list(range(n)), list(range(n))[::-1], [3, 5, 0, 2, 6, 1, 4]):
                for nfixed in (0, 2):
                    order, cards = be.greedy_cards([paths[i] for i in listed], mode, nfixed, n, kmin)
                    worder, wcards = _oracle_walk(orc, leaf, p, kmin, code, listed, nfixed, n)
                    assert [listed[i] for i in order] == [int(x) for x in worder], (mode, listed, nfixed)
                    assert np.array_equal(cards, wcards)
                    first, second = (2, 5) if listed.index(2) < listed.index(5) else (5, 2)
                    seq = [listed[i] for i in order]
                    assert seq.index(first) < seq.index(second)
        assert len(uploads) == 1 and be._dev is not None          # one slab for every call, whatever order the leaves came in
        held = be._dev[1]
        be.leave_out_cards(paths, np.arange(n))
        be.pairwise_cards(paths)
        assert len(uploads) == 1 and be._dev[1] == held
        os.environ["DANDD_DEVICE_CACHE_MB"] = "0"                  # host slab: dd_greedy's host-pointer form
        try:
            order, cards = be.greedy_cards(paths, "max", 1, n - 1, kmin)
            worder, wcards = _oracle_walk(orc, leaf, p, kmin, 0, list(range(n)), 1, n - 1)
            assert np.array_equal(order, worder) and np.array_equal(cards, wcards)
        finally:
            del os.environ["DANDD_DEVICE_CACHE_MB"]
    finally:
        be.close()


def test_exact_tree_table_path_equals_object_path(tmp_path, torch_cuda):
    """An --exact tree of the five golden FASTAs: the walk over the GPU's subset table == one SubSpider per step and candidate."""
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    t = str(tmp_path / "t")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "tree", "-d", data, "-o", t, "-s", "gold", "-k", "10", "--exact"],
                   env=env, check=True, cwd=ROOT, timeout=600, capture_output=True)
    (pk,) = glob.glob(os.path.join(t, "*dtree.pickle"))
    out = {}
    for name, extra in (("table", []), ("object", ["--safe"])):
        d = str(tmp_path / name)
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "greedy", "-d", pk, "-o", d, "--ksweep", "--mink", "8",
                            "--maxk", "16", *extra], env=env, cwd=ROOT, timeout=600, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = _greedy_files(d)
    assert len(out["table"]) == 4 and out["table"] == out["object"]


def test_size_64_genomes_log2m_20(engine_factory, torch_cuda):
    """64 x 5 Mbp synthetic genomes, -r 20, k 10..40 through the device slab.  dd_greedy_device in both modes == the walk over
    dd_extend_device rows; the last step's cards == the root union's; device time, bytes and rate are printed.  One assertion
    on time: the call is faster than the same walk emulated with one dd_progressive_device call per step."""
    from dandd_amd.engine import synth_size
    p, n, kmin, kmax = 20, 64, 10, 40
    K = kmax - kmin + 1
    eng = engine_factory(log2m=p)
    torch = torch_cuda
    slab = torch.empty((n, K, 1 << p), dtype=torch.uint8, device="cuda")
    for lo in range(0, n, 16):
        bufs, sizes = [], []
        for gi in range(lo, lo + 16):
            size = synth_size(5_000_000, 4)
            t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
            eng.synth_fasta_device(0xD4ADD, gi, 5_000_000, 4, t.data_ptr())
            bufs.append(t)
            sizes.append(size)
        eng.sketch_device([b.data_ptr() for b in bufs], sizes, kmin, kmax, slab[lo].data_ptr())
        eng.synchronize()
        del bufs
    ptr = slab.data_ptr()
    ks = list(range(kmin, kmax + 1))
    eng.greedy_device(ptr, n, K, kmin, 0, nsteps=2)             # (first launches)
    got = {}
    for mode in (0, 1):
        eng.timing_enable(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        got[mode] = eng.greedy_device(ptr, n, K, kmin, mode)
        wall = time.perf_counter() - t0
        ms, launches = eng.timing_read(2)
        eng.timing_enable(False)
        gbytes = sum(n - j for j in range(n)) * K * (1 << p) / 1e9
        print(f"\ngreedy {'max' if mode == 0 else 'min'} 64 x 5 Mbp, log2m 20, k 10..40: {ms:.3f} ms device ({launches} spans), "
              f"{wall * 1e3:.2f} ms call; {gbytes:.2f} GB of candidate rows -> {gbytes / ms:.2f} TB/s")
        got[mode] = got[mode] + (wall,)
    # the walk over dd_extend_device rows, the running union kept by torch
    for mode in (0, 1):
        order, cards, _ = got[mode]
        left, base = list(range(n)), None
        for j in range(n):
            rows = eng.extend_device(base.data_ptr() if j else 0, ptr, n, K, left)
            ds = [_delta(r, ks) for r in rows]
            pick = 0
            for r in range(1, len(left)):
                if (ds[r] > ds[pick]) if mode == 0 else (ds[r] < ds[pick]):
                    pick = r
            assert left[pick] == order[j], (mode, j)
            assert np.array_equal(rows[pick], cards[j]), (mode, j)
            c = left.pop(pick)
            base = slab[c].clone() if base is None else torch.maximum(base, slab[c])
    out = torch.empty(1 << p, dtype=torch.uint8, device="cuda")
    for kk in (0, 10, K - 1):
        eng.union_device([slab[i, kk].data_ptr() for i in range(n)], 1 << p, out.data_ptr())
        root = eng.card_batch_device(out.data_ptr(), 1)[0]
        assert root == got[0][1][n - 1, kk] == got[1][1][n - 1, kk]
    # the emulation: per step one ordering (chosen..., g, rest...) per candidate g, of which only prefix j + 1 is wanted
    order, cards, wall = got[0]
    eng.progressive_device(ptr, n, K, [list(range(n))])        # (first launch)
    t0 = time.perf_counter()
    chosen, left = [], list(range(n))
    for j in range(n):
        ords = [chosen + [g] + [x for x in left if x != g] for g in left]
        rows = eng.progressive_device(ptr, n, K, ords)[:, j, :]
        ds = [_delta(r, ks) for r in rows]
        pick = 0
        for r in range(1, len(left)):
            if ds[r] > ds[pick]:
                pick = r
        assert np.array_equal(rows[pick], cards[j]), j
        chosen.append(left.pop(pick))
    emulated = time.perf_counter() - t0
    assert chosen == [int(x) for x in order]
    print(f"greedy max by one dd_progressive_device call per step: {emulated * 1e3:.1f} ms; dd_greedy_device: {wall * 1e3:.2f} ms "
          f"({emulated / wall:.1f} x)")
    assert wall < emulated
