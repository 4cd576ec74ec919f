"""dd_subsets on the MI355X: the union of every subset of n <= 16 leaves from threshold bit planes (dd_subsets.hip), against
the oracle's card of a numpy byte-max over each subset -- doubles compared with ==; the backend's row remapping, and the
`dandd abba` CLI against the CPU checker and through `dandd serve`."""
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
        leaf = np.minimum(rng.geometric(0.5, size=(n, K, m)), 64 - p + 1).astype(np.uint8)
    elif kind == "two-values":
        leaf = rng.integers(7, 9, size=(n, K, m), dtype=np.uint8)
    elif kind == "identical":
        one = np.minimum(rng.geometric(0.5, size=(1, K, m)), 30).astype(np.uint8)
        leaf = np.repeat(one, n, axis=0)
    elif kind == "zeros":
        leaf = np.minimum(rng.geometric(0.5, size=(n, K, m)), 30).astype(np.uint8)
        leaf[: max(1, n // 2)] = 0
    else:
        raise ValueError(kind)
    # the last column spans the whole byte range: 0 and 63 both in it (T = 63 thresholds)
    leaf[:, K - 1, : m // 2] = 0
    leaf[n - 1, K - 1, m // 2:] = 63
    return leaf


def _masks(rng, n):
    """every subset for n <= 7; else every singleton, the full set, every complement of a singleton and 64 seeded masks
    per subset size"""
    full = (1 << n) - 1
    if n <= 7:
        return list(range(1 << n))
    out = {full} | {1 << i for i in range(n)} | {full ^ (1 << i) for i in range(n)}
    for size in range(1, n + 1):
        for _ in range(64):
            out.add(int(sum(1 << int(i) for i in rng.choice(n, size=size, replace=False))))
    return sorted(out)


def _check(orc, leaf, got, masks, p):
    n, K, _ = leaf.shape
    assert got.shape == (1 << n, K)
    assert np.array_equal(got[0], np.zeros(K))
    for s in masks:
        if s == 0:
            continue
        rows = [i for i in range(n) if s >> i & 1]
        for kk in range(K):
            want = orc.card(np.max(leaf[rows, kk], axis=0), p)
            assert got[s, kk] == want, (n, K, p, s, kk, got[s, kk], want)


CASES = [(n, K, p) for n in (1, 2, 5, 6, 7, 12, 13, 16) for p in (4, 10, 14, 17, 20) for K in (1, 3)]


@pytest.mark.parametrize("n,K,p", CASES)
def test_subsets_match_oracle(engine_factory, orc, n, K, p):
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(n * 1000 + K * 10 + p)
    leaf = _leaf(rng, n, K, p, "random")
    _check(orc, leaf, eng.subsets(leaf), _masks(rng, n), p)


@pytest.mark.parametrize("kind", ["two-values", "identical", "zeros"])
@pytest.mark.parametrize("n,K,p", [(1, 1, 4), (5, 3, 10), (7, 3, 4), (13, 1, 14), (16, 3, 17)])
def test_subsets_ties(engine_factory, orc, kind, n, K, p):
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(11 + n)
    leaf = _leaf(rng, n, K, p, kind)
    _check(orc, leaf, eng.subsets(leaf), _masks(rng, n), p)


def test_subsets_errors(engine_factory):
    from dandd_amd.engine import EngineError
    eng = engine_factory(log2m=10)
    with pytest.raises(EngineError, match="outside 1..16"):
        eng.subsets(np.zeros((17, 1, 1 << 10), dtype=np.uint8))
    with pytest.raises(EngineError, match="outside 1..16"):
        eng.subsets(np.zeros((0, 1, 1 << 10), dtype=np.uint8))


def test_device_slab_and_backend_permutation(engine_factory, torch_cuda, orc, tmp_path):
    p, n, K = 14, 9, 4
    eng = engine_factory(log2m=p)
    rng = np.random.default_rng(3)
    leaf = _leaf(rng, n, K, p, "random")
    host = eng.subsets(leaf)
    dev = torch_cuda.from_numpy(leaf).cuda()
    assert np.array_equal(eng.subsets_device(dev.data_ptr(), n, K), host)
    _check(orc, leaf, host, _masks(rng, n), p)
    # HipBackend: leaves listed out of sorted order (the device slab keeps them sorted by path: a permutation of the masks)
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
        assert np.array_equal(be.subset_cards(paths), host)
        assert np.array_equal(be.subset_cards(paths), host)                # (second call: the slab already in HBM)
        os.environ["DANDD_DEVICE_CACHE_MB"] = "0"                          # host slab
        try:
            assert np.array_equal(be.subset_cards(paths), host)
        finally:
            del os.environ["DANDD_DEVICE_CACHE_MB"]
    finally:
        be.close()


def test_size_16_genomes_log2m_20(engine_factory, torch_cuda, orc):
    """16 x 5 Mbp synthetic genomes, -r 20, k 10..40 through the device slab: sampled subsets against the oracle; the
    kernel's time is printed, not asserted."""
    from dandd_amd.engine import synth_size
    p, n, kmin, kmax = 20, 16, 10, 40
    K = kmax - kmin + 1
    eng = engine_factory(log2m=p)
    torch = torch_cuda
    slab = torch.empty((n, K, 1 << p), dtype=torch.uint8, device="cuda")
    bufs, sizes = [], []
    for gi in range(n):
        size = synth_size(5_000_000, 4)
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(0xD4ADD, gi, 5_000_000, 4, t.data_ptr())
        bufs.append(t)
        sizes.append(size)
    eng.sketch_device([b.data_ptr() for b in bufs], sizes, kmin, kmax, slab.data_ptr())
    eng.synchronize()
    del bufs
    eng.subsets_device(slab.data_ptr(), n, K)                 # (first launch)
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    got = eng.subsets_device(slab.data_ptr(), n, K)
    wall = time.perf_counter() - t0
    ms, launches = eng.timing_read(2)
    eng.timing_enable(False)
    print(f"\nsubsets 16 x 5 Mbp, log2m 20, k {kmin}..{kmax}: {ms:.3f} ms device ({launches} spans), {wall * 1e3:.2f} ms call")
    host = slab.cpu().numpy()
    rng = np.random.default_rng(5)
    full = (1 << n) - 1
    masks = [full, 1, 1 << 15, full ^ 1] + [int(x) for x in rng.integers(1, full, size=6)]
    for s in masks:
        rows = [i for i in range(n) if s >> i & 1]
        for kk in (0, 13, K - 1):
            assert got[s, kk] == orc.card(np.max(host[rows, kk], axis=0), p), (s, kk)


@pytest.mark.parametrize("regs", [14, 20])
def test_cli_end_to_end(tmp_path, regs, sock_dir, torch_cuda):
    """`abba` with HipBackend == the CPU checker's files, byte for byte; the same command through `dandd serve` + the client
    writes the same bytes."""
    from dandd_amd.host import cli, deltatree
    import test_abba as cpu
    import test_deltadelta as ddcpu
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    t = str(tmp_path / "t")
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "tree", "-d", data, "-o", t, "-s", "gold", "-k", "10", "-r",
                    str(regs)], env=env, check=True, cwd=ROOT, timeout=300, capture_output=True)
    pk = os.path.join(t, "gold_5_dashing_dtree.pickle")
    argv = ["--subsets", "--ksweep", "--mink", "8", "--maxk", "16"]
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "abba", "-d", pk, "-o", one, *argv], env=env, cwd=ROOT,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deltatree.set_backend_factory(lambda r_, c: hostcheck.OracleBackend(r_, c))
    try:
        _, pkc = ddcpu._tree(str(tmp_path / "cpu"), deltatree, registers=regs)
        deltatree.set_backend_factory(lambda r_, c: cpu.SubsetBackend(r_, c))
        cli.main(["abba", "-d", pkc, "-o", str(tmp_path / "cpu" / "ab"), *argv])
    finally:
        deltatree.set_backend_factory(None)
    cpu_data = os.path.join(str(tmp_path / "cpu"), "data")
    for name in cpu.FILES:
        with open(os.path.join(one, f"gold_5_dashing.{name}.csv")) as a, \
                open(os.path.join(str(tmp_path / "cpu" / "ab"), f"gold_5_dashing.{name}.csv")) as b:
            assert a.read().replace(data, "D") == b.read().replace(cpu_data, "D"), name
    sock = os.path.join(sock_dir, "ab.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", "abba", "-d", pk, "-o", via, *argv], env=cenv,
                           cwd=ROOT, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for name in cpu.FILES:
            with open(os.path.join(one, f"gold_5_dashing.{name}.csv"), "rb") as a, \
                    open(os.path.join(via, f"gold_5_dashing.{name}.csv"), "rb") as b:
                assert a.read() == b.read(), name
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()
