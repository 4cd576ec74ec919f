"""dd_leave_out on the MI355X: every "union of all leaves but group g" from one pass over the leaf slab (dd_leaveout.hip),
against the oracle's card of a numpy byte-max over each complement -- doubles compared with ==; the backend and CLI paths
(`dandd deltadelta`) against the CPU checker, the reference's own find_delta_delta values and `dandd serve`."""
import csv
import json
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


def _leaf(rng, n, K, p, kind):
    m = 1 << p
    if kind == "random":
        return np.minimum(rng.geometric(0.5, size=(n, K, m)), 64 - p + 1).astype(np.uint8)
    if kind == "two-values":
        return rng.integers(7, 9, size=(n, K, m), dtype=np.uint8)
    if kind == "identical":
        one = np.minimum(rng.geometric(0.5, size=(1, K, m)), 30).astype(np.uint8)
        return np.repeat(one, n, axis=0)
    if kind == "zeros":
        leaf = np.minimum(rng.geometric(0.5, size=(n, K, m)), 30).astype(np.uint8)
        leaf[: max(1, n // 2)] = 0
        return leaf
    raise ValueError(kind)


def _groupings(rng, n):
    """name -> group[n]: singletons, a random partition, one large group + singletons, floor (-1) leaves"""
    out = {"singletons": np.arange(n)}
    if n >= 3:
        g = rng.integers(0, max(2, n // 3), size=n)
        g[0], g[1] = 0, 1                                          # no group may hold every leaf
        _, g = np.unique(g, return_inverse=True)
        out["partition"] = g
        big = np.zeros(n, dtype=np.int64)
        big[n // 2:] = np.arange(1, n - n // 2 + 1)
        out["large+singletons"] = big
        fl = np.arange(n) - 1
        fl[0] = -1
        fl[1::3] = -1
        fl[fl >= 0] = np.arange((fl >= 0).sum())
        out["floor"] = fl
    return out


def _want(orc, leaf, group, p):
    """oracle card of a byte-max over every complement: prefix/suffix maxima for singletons, a direct max for groups"""
    n, K, _ = leaf.shape
    G = int(group.max()) + 1
    out = np.empty((G + 1, K))
    singles = all((group == g).sum() == 1 for g in range(G)) and (group >= 0).all()
    for kk in range(K):
        col = leaf[:, kk]
        full = col.max(axis=0)
        out[G, kk] = orc.card(full, p)
        if singles:
            pre = np.maximum.accumulate(col, axis=0)
            suf = np.maximum.accumulate(col[::-1], axis=0)[::-1]
            for i in range(n):
                parts = ([pre[i - 1]] if i > 0 else []) + ([suf[i + 1]] if i + 1 < n else [])
                out[group[i], kk] = orc.card(np.maximum.reduce(parts), p)
        else:
            for g in range(G):
                out[g, kk] = orc.card(col[group != g].max(axis=0), p)
    return out


CASES = [(n, K, p) for n in (2, 3, 17, 64) for K in (1, 5, 37) for p in (10, 14, 16, 20)
         if n <= 3 or n * K * (1 << p) <= (1 << 25)] + [(300, 1, 10), (300, 5, 14), (300, 5, 12)]


@pytest.mark.parametrize("n,K,p", CASES)
def test_leave_out_matches_oracle(engine_factory, orc, n, K, p):
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(n * 1000 + K * 10 + p)
    leaf = _leaf(rng, n, K, p, "random")
    for name, group in _groupings(rng, n).items():
        got = eng.leave_out(leaf, group)
        assert np.array_equal(got, _want(orc, leaf, group, p)), (name, n, K, p)


@pytest.mark.parametrize("kind", ["two-values", "identical", "zeros"])
@pytest.mark.parametrize("n,K,p", [(2, 1, 10), (17, 5, 14), (64, 3, 16), (300, 2, 12)])
def test_leave_out_ties(engine_factory, orc, kind, n, K, p):
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(7 + n)
    leaf = _leaf(rng, n, K, p, kind)
    for name, group in _groupings(rng, n).items():
        assert np.array_equal(eng.leave_out(leaf, group), _want(orc, leaf, group, p)), (kind, name)
    # the maximum held by two groups everywhere: leaving either out changes nothing
    if n >= 4:
        leaf2 = leaf.copy()
        leaf2[1] = leaf2[0] = np.maximum(leaf[0], 40)
        group = np.arange(n)
        got = eng.leave_out(leaf2, group)
        assert np.array_equal(got, _want(orc, leaf2, group, p))
        assert np.array_equal(got[0], got[n]) and np.array_equal(got[1], got[n])


def test_leave_out_errors(engine_factory):
    from dandd_amd.engine import EngineError
    eng = engine_factory(log2m=10)
    leaf = np.zeros((3, 2, 1 << 10), dtype=np.uint8)
    with pytest.raises(EngineError, match="outside"):
        eng.leave_out(leaf, [0, 1, 5], ngroups=2)
    with pytest.raises(EngineError, match="at least one group"):
        eng.leave_out(leaf, [-1, -1, -1], ngroups=0)
    with pytest.raises(EngineError, match="every leaf"):
        eng.leave_out(leaf, [0, 0, 0])


def test_device_slab_and_backend_permutation(engine_factory, torch_cuda, orc, tmp_path):
    p, n, K = 14, 9, 4
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(3)
    leaf = _leaf(rng, n, K, p, "random")
    group = np.array([0, 1, -1, 2, 1, 3, -1, 4, 5])
    host = eng.leave_out(leaf, group)
    dev = torch_cuda.from_numpy(leaf).cuda()
    assert np.array_equal(eng.leave_out_device(dev.data_ptr(), n, K, group), host)
    assert np.array_equal(host, _want(orc, leaf, group, p))
    # HipBackend: leaves listed out of sorted order (the device slab keeps them sorted by path: a permutation)
    from dandd_amd.host.backend import HipBackend, write_sketch_file
    be = HipBackend(log2m=p)
    try:
        paths = []
        for i in range(n):
            row = []
            for kk in range(K):
                path = str(tmp_path / f"leaf{(7 * i) % n}_{i}.k{kk + 5}.hll")
                write_sketch_file(path, leaf[i, kk], p, kk + 5, True)
                row.append(path)
            paths.append(row)
        order = sorted(range(n), key=lambda i: paths[i][0])
        assert order != list(range(n))
        assert np.array_equal(be.leave_out_cards(paths, group), host)
        assert np.array_equal(be.leave_out_cards(paths, group), host)          # (second call: the slab already in HBM)
        os.environ["DANDD_DEVICE_CACHE_MB"] = "0"                              # host slab
        try:
            assert np.array_equal(be.leave_out_cards(paths, group), host)
        finally:
            del os.environ["DANDD_DEVICE_CACHE_MB"]
    finally:
        be.close()


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


@pytest.mark.parametrize("regs", [14, 20])
def test_cli_end_to_end(tmp_path, regs, sock_dir, torch_cuda):
    """`deltadelta` with HipBackend == the CPU checker's rows (and, at -r 14, the reference's find_delta_delta values); the
    same command through `dandd serve` + the client writes the same bytes."""
    from dandd_amd.host import cli, deltatree
    import test_deltadelta as cpu
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    t = str(tmp_path / "t")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "tree", "-d", data, "-o", t, "-s", "gold", "-k", "10", "-r",
                    str(regs)], env=env, check=True, cwd=ROOT, timeout=300, capture_output=True)
    pk = os.path.join(t, "gold_5_dashing_dtree.pickle")
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "deltadelta", "-d", pk, "-o", one], env=env, cwd=ROOT,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = _rows(os.path.join(one, "gold_5_dashing.deltadelta.csv"))
    # the CPU checker: the same tree built and asked again from scratch, in a directory of its own
    deltatree.set_backend_factory(lambda r_, c: hostcheck.OracleBackend(r_, c))
    try:
        _, pkc = cpu._tree(str(tmp_path / "cpu"), deltatree, registers=regs)
        deltatree.set_backend_factory(lambda r_, c: cpu.LeaveOutBackend(r_, c))
        cli.main(["deltadelta", "-d", pkc, "-o", str(tmp_path / "cpu" / "dd")])
    finally:
        deltatree.set_backend_factory(None)
    want = _rows(os.path.join(str(tmp_path / "cpu" / "dd"), "gold_5_dashing.deltadelta.csv"))

    def plain(rows):
        return [dict(r, fastas=[os.path.basename(f) for f in r["fastas"].split("|")]) for r in rows]
    assert plain(got) == plain(want)
    if regs == 14:
        with open(os.path.join(hostcheck.GOLD, "ref_deltadelta.json")) as f:
            gold = json.load(f)
        assert [float(x["deltadelta"]) for x in got] == [g["deltadelta"] for g in gold["groups"]]
        assert [float(x["delta_rest"]) for x in got] == [g["subtree_delta"] for g in gold["groups"]]
    # through a resident server
    sock = os.path.join(sock_dir, "dd.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", "deltadelta", "-d", pk, "-o", via], env=cenv,
                           cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        with open(os.path.join(one, "gold_5_dashing.deltadelta.csv"), "rb") as a, \
                open(os.path.join(via, "gold_5_dashing.deltadelta.csv"), "rb") as b:
            assert a.read() == b.read()
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()


def test_size_64_genomes_log2m_20(engine_factory, torch_cuda):
    """64 x 5 Mbp synthetic genomes, -r 20, k 4..32 through the device slab: 3 sampled complements against the streaming
    union + card; the kernel's time is printed, not asserted."""
    from dandd_amd.engine import synth_size
    p, n, kmin, kmax = 20, 64, 4, 32
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
    group = np.arange(n)
    eng.leave_out_device(slab.data_ptr(), n, K, group)        # (first launch)
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    got = eng.leave_out_device(slab.data_ptr(), n, K, group)
    wall = time.perf_counter() - t0
    ms, launches = eng.timing_read(2)
    eng.timing_enable(False)
    gbytes = n * K * (1 << p) / 1e9
    print(f"\nleave-out 64 x 5 Mbp, log2m 20, k 4..32: {ms:.3f} ms device ({launches} spans), {wall * 1e3:.2f} ms call; "
          f"{gbytes:.2f} GB slab -> {gbytes / ms:.2f} TB/s ({gbytes / 5.6 / ms:.2f} of 5.6 TB/s)")
    out = torch.empty(1 << p, dtype=torch.uint8, device="cuda")
    for g in (0, 31, 63):
        for kk in (0, 10, K - 1):
            ins = [slab[i, kk].data_ptr() for i in range(n) if i != g]
            eng.union_device(ins, 1 << p, out.data_ptr())
            assert eng.card_batch_device(out.data_ptr(), 1)[0] == got[g, kk], (g, kk)
    for kk in (0, K - 1):
        eng.union_device([slab[i, kk].data_ptr() for i in range(n)], 1 << p, out.data_ptr())
        assert eng.card_batch_device(out.data_ptr(), 1)[0] == got[n, kk]
