"""`dandd greedy` on the CPU: the steepest and the flattest growth ordering.

The schedule path (one greedy_cards call per mode, here a brute-force oracle union + card per step and candidate) is
checked against the object path (one SubSpider per step and candidate) and the subset-table path (a walk over subset_cards),
against `abba --subsets`, against `progressive` replaying the written ordering and all 120 orderings of the five golden
FASTAs, and for its tie rule, its argument errors and the server."""
import ast
import csv
import glob
import io
import math
import os
import shutil
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import test_abba as ab
import test_deltadelta as dd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "server_worker.py")
WINDOW = ab.WINDOW
KS = list(range(8, 17))


def _delta(cards, ks):
    """the rule as the issue states it, written out here on its own: largest card / k, a later k winning a tie"""
    best, bestk = 0, 0
    for c, k in zip(cards, ks):
        if c / k >= best:
            best, bestk = c / k, k
    return best, bestk


def _walk(card_of, n, nfixed, nsteps, mode, ks):
    """items 0..nfixed-1 given, then the best remaining item by _delta, the earlier item winning a tie"""
    order, cards, left = [], [], list(range(nfixed, n))
    for j in range(nsteps):
        rows = [j] if j < nfixed else left
        got = [card_of(order, c) for c in rows]
        ds = [_delta(g, ks)[0] for g in got]
        pick = 0
        for r in range(1, len(rows)):
            if (ds[r] > ds[pick]) if mode == "max" else (ds[r] < ds[pick]):
                pick = r
        order.append(rows[pick])
        cards.append(got[pick])
        if j >= nfixed:
            left.pop(pick)
    return order, cards


class GreedyBackend(hostcheck.ScheduleBackend):
    """The schedule backend with greedy_cards, brute force: oracle union + oracle card per step and candidate."""
    name = "oracle+greedy"
    calls = 0

    def greedy_cards(self, leaf_paths, mode, nfixed, nsteps, kmin):
        GreedyBackend.calls += 1
        slab = self._slab(leaf_paths)
        n, K = len(slab), len(slab[0])
        ks = list(range(kmin, kmin + K))

        def card_of(chosen, c):
            return [self.orc.card(self.orc.union(*[slab[i][kk] for i in list(chosen) + [c]]), self.log2m) for kk in range(K)]
        order, cards = _walk(card_of, n, nfixed, nsteps, mode, ks)
        return np.array(order), np.array(cards)


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)


def _greedy(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["greedy", *argv])


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _outputs(d):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(d, "*greedy*"))}


@pytest.mark.parametrize("regs", [14, 20])
def test_three_paths_write_the_same_bytes(host, tmp_path, regs):
    data, pk = dd._tree(str(tmp_path), host, registers=regs)
    basef = tmp_path / "base.txt"
    basef.write_text(os.path.join(data, "g3.fasta") + "\ng1.fasta\n")
    configs = [(["--mode", "both"], ["max", "min"], 5),
               (["--mode", "max", "-b", str(basef), "--steps", "4"], ["max"], 4),
               (["--mode", "min", "--steps", "3"], ["min"], 3),
               (["--mode", "both", "-b", str(basef)], ["max", "min"], 5)]
    for ci, (extra, modes, steps) in enumerate(configs):
        got = {}
        for name, backend in (("sched", GreedyBackend), ("object", hostcheck.ScheduleBackend), ("table", ab.SubsetBackend)):
            o = str(tmp_path / f"{name}{ci}")
            calls, tables = GreedyBackend.calls, ab.SubsetBackend.calls
            _greedy(host, backend, ["-d", pk, "-o", o, *WINDOW, *extra])
            if name == "sched":
                assert GreedyBackend.calls == calls + len(modes)       # exactly one greedy_cards call per mode
            if name == "table":
                assert ab.SubsetBackend.calls == tables + 1            # one subset table for every mode
            got[name] = _outputs(o)
        want = {"gold_5_dashing.greedy.csv", "gold_5_dashing.greedysummary.csv"} | {f"gold_5_dashing.greedy_{m}.txt" for m in modes}
        assert set(got["sched"]) == want
        assert got["sched"] == got["object"] == got["table"], (regs, extra)
        rows = _rows(os.path.join(str(tmp_path / f"sched{ci}"), "gold_5_dashing.greedy.csv"))
        assert len(rows) == steps * len(modes)
        for m in modes:
            mine = [r for r in rows if r["mode"] == m]
            assert [int(r["ngen"]) for r in mine] == list(range(1, steps + 1))
            if "-b" in extra:
                assert [os.path.basename(r["fasta"]) for r in mine[:2]] == ["g3.fasta", "g1.fasta"]
            prev = 0.0
            for j, r in enumerate(mine):
                assert float(r["gain"]) == float(r["delta"]) - prev
                prev = float(r["delta"])
                assert r["fastas"].split("|") == [x["fasta"] for x in mine[:j + 1]]
            lines = open(os.path.join(str(tmp_path / f"sched{ci}"), f"gold_5_dashing.greedy_{m}.txt")).read().splitlines()
            assert lines == [r["fasta"] for r in mine]
        summ = _rows(os.path.join(str(tmp_path / f"sched{ci}"), "gold_5_dashing.greedysummary.csv"))
        assert len(summ) == steps * len(modes) * len(KS)
        for r in summ:
            assert float(r["delta_pos"]) == float(r["card"]) / int(r["kval"])


def test_against_abba_subsets(host, tmp_path):
    data, pk = dd._tree(str(tmp_path), host)
    a, g = str(tmp_path / "a"), str(tmp_path / "g")
    ab._abba(host, ab.SubsetBackend, ["-d", pk, "-o", a, "--subsets", *WINDOW])
    _greedy(host, GreedyBackend, ["-d", pk, "-o", g, *WINDOW])
    sub = {int(r["mask"]): r for r in _rows(os.path.join(a, "gold_5_dashing.abba_subsets.csv"))}
    fastas = [sub[1 << i]["fastas"] for i in range(5)]
    rows = _rows(os.path.join(g, "gold_5_dashing.greedy.csv"))
    for mode in ("max", "min"):
        mine = [r for r in rows if r["mode"] == mode]
        mask = 0
        for r in mine:
            cands = [i for i in range(5) if not mask >> i & 1]
            ds = [float(sub[mask | 1 << c]["delta"]) for c in cands]
            pick = 0
            for i in range(1, len(cands)):
                if (ds[i] > ds[pick]) if mode == "max" else (ds[i] < ds[pick]):
                    pick = i
            c = cands[pick]
            assert r["fasta"] == fastas[c]
            assert float(r["delta"]) == ds[pick] and int(r["kval"]) == int(sub[mask | 1 << c]["kval"])
            assert all(ds[pick] >= d for d in ds) if mode == "max" else all(ds[pick] <= d for d in ds)
            mask |= 1 << c
        assert mask == 31


def _progressive_tables(host, pk, out, backend, extra):
    from dandd_amd.host import cli
    os.makedirs(out, exist_ok=True)
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["progressive", "-d", pk, "-o", out, *WINDOW, *extra])
    tables = [_rows(f) for f in sorted(glob.glob(os.path.join(out, "*progu*.csv")))]
    summ = next(t for t in tables if t and "card" in t[0] and "ordering" in t[0])
    res = next(t for t in tables if t and "fastas" in t[0] and "ordering" in t[0])
    cards = {}
    for r in summ:
        cards.setdefault((int(r["ordering"]), int(r["ngen"])), []).append((int(r["kval"]), float(r["card"])))
    for kc in cards.values():
        kc.sort()
    prefix = {}
    for r in res:
        cell = r["fastas"]
        prefix[(int(r["ordering"]), int(r["ngen"]))] = ast.literal_eval(cell) if cell.startswith("[") else cell.split("|")
    return cards, prefix


def test_against_progressive(host, tmp_path):
    from dandd_amd.host.deltatree import _window_delta
    data, pk = dd._tree(str(tmp_path), host)
    g = str(tmp_path / "g")
    _greedy(host, GreedyBackend, ["-d", pk, "-o", g, *WINDOW])
    rows = _rows(os.path.join(g, "gold_5_dashing.greedy.csv"))
    summ = _rows(os.path.join(g, "gold_5_dashing.greedysummary.csv"))
    # `progressive -f greedy_max.txt -n 1` replays the ordering: the same cards, and delta / kval rebuilt from them
    cards, prefix = _progressive_tables(host, pk, str(tmp_path / "replay"), hostcheck.ScheduleBackend,
                                        ["-f", os.path.join(g, "gold_5_dashing.greedy_max.txt"), "-n", "1"])
    (o,) = {key[0] for key in cards}
    mine = [r for r in rows if r["mode"] == "max"]
    for r in mine:
        ng = int(r["ngen"])
        kc = cards[(o, ng)]
        assert [(int(s["kval"]), float(s["card"])) for s in summ if s["mode"] == "max" and int(s["ngen"]) == ng] == kc
        assert _window_delta([c for _, c in kc], [k for k, _ in kc]) == (float(r["delta"]), int(r["kval"]))
        assert set(prefix[(o, ng)]) == set(r["fastas"].split("|"))
    # all 120 orderings: among those that share greedy's first j genomes none does better at step j + 1
    cards, prefix = _progressive_tables(host, pk, str(tmp_path / "all"), hostcheck.ScheduleBackend, ["-n", str(math.factorial(5))])
    orders = sorted({key[0] for key in cards})
    assert len(orders) == 120
    delta = {key: _window_delta([c for _, c in kc], [k for k, _ in kc])[0] for key, kc in cards.items()}
    for mode in ("max", "min"):
        mine = [r for r in rows if r["mode"] == mode]
        for j in range(5):
            start = set(mine[j]["fastas"].split("|")) - {mine[j]["fasta"]}
            peers = [o for o in orders if j == 0 or set(prefix[(o, j)]) == start]
            assert len(peers) == math.factorial(j) * math.factorial(5 - j)
            mined = float(mine[j]["delta"])
            for o in peers:
                assert delta[(o, j + 1)] <= mined if mode == "max" else delta[(o, j + 1)] >= mined


def test_ties_follow_the_order_of_the_fasta_list(host, tmp_path):
    from dandd_amd.host import cli
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    shutil.copyfile(os.path.join(data, "g1.fasta"), os.path.join(data, "twin.fasta"))    # the same bytes under another name
    out = str(tmp_path / "t")
    os.makedirs(out)
    host.set_backend_factory(lambda r, c: hostcheck.OracleBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", out, "-s", "gold", "-k", "10", "-r", "12"])
    pk = os.path.join(out, "gold_6_dashing_dtree.pickle")
    names = ["g0.fasta", "g1.fasta", "g2.fasta", "twin.fasta", "g3.fasta", "g4.fasta"]
    fwd, rev = tmp_path / "fwd.txt", tmp_path / "rev.txt"
    fwd.write_text("".join(os.path.join(data, n) + "\n" for n in names))
    rev.write_text("".join(os.path.join(data, n) + "\n" for n in reversed(names)))
    swap = {"g1.fasta": "twin.fasta", "twin.fasta": "g1.fasta"}
    for backend in (GreedyBackend, hostcheck.ScheduleBackend, ab.SubsetBackend):
        a, b = str(tmp_path / (backend.name + "_a")), str(tmp_path / (backend.name + "_b"))
        _greedy(host, backend, ["-d", pk, "-o", a, "-f", str(fwd), *WINDOW])
        _greedy(host, backend, ["-d", pk, "-o", b, "-f", str(rev), *WINDOW])
        for mode in ("max", "min"):
            first = [os.path.basename(x) for x in open(os.path.join(a, f"gold_6_dashing.greedy_{mode}.txt")).read().splitlines()]
            second = [os.path.basename(x) for x in open(os.path.join(b, f"gold_6_dashing.greedy_{mode}.txt")).read().splitlines()]
            assert sorted(first) == sorted(names)
            assert first.index("g1.fasta") < first.index("twin.fasta")        # g1 stands first in fwd.txt
            assert second.index("twin.fasta") < second.index("g1.fasta")      # ... twin in rev.txt
            assert second == [swap.get(x, x) for x in first]                  # and nothing else moves
        ra, rb = _rows(os.path.join(a, "gold_6_dashing.greedy.csv")), _rows(os.path.join(b, "gold_6_dashing.greedy.csv"))
        assert [(r["mode"], r["ngen"], r["delta"], r["kval"], r["gain"]) for r in ra] == \
            [(r["mode"], r["ngen"], r["delta"], r["kval"], r["gain"]) for r in rb]


def test_errors(host, tmp_path):
    data, pk = dd._tree(str(tmp_path), host)
    e = tmp_path / "e"

    def fails(argv, text):
        with pytest.raises(SystemExit) as err:
            _greedy(host, GreedyBackend, ["-d", pk, "-o", str(e), *argv])
        assert isinstance(err.value.code, str) and text in err.value.code and "\n" not in err.value.code, (argv, err.value.code)
        assert not glob.glob(os.path.join(str(e), "*greedy*"))
    fails([], "a k window is needed")
    outside = tmp_path / "outside.txt"
    outside.write_text(os.path.join(data, "g4.fasta") + "\n")
    uni = tmp_path / "uni.txt"
    uni.write_text("".join(os.path.join(data, n) + "\n" for n in dd.NAMES[:4]))
    fails([*WINDOW, "-f", str(uni), "-b", str(outside)], "not in the universe")
    nowhere = tmp_path / "nowhere.txt"
    nowhere.write_text("nowhere.fasta\n")
    fails([*WINDOW, "-b", str(nowhere)], "not a leaf")
    twice = tmp_path / "twice.txt"
    twice.write_text("g2.fasta\n" + os.path.join(data, "g2.fasta") + "\n")
    fails([*WINDOW, "-b", str(twice)], "twice")
    fails([*WINDOW, "--steps", "0"], "--steps 0")
    fails([*WINDOW, "--steps", "6"], "--steps 6")
    two = tmp_path / "two.txt"
    two.write_text("g2.fasta\ng0.fasta\n")
    fails([*WINDOW, "-b", str(two), "--steps", "1"], "fewer than the 2")
    one = tmp_path / "one.txt"
    one.write_text(os.path.join(data, "g2.fasta") + "\n")
    fails([*WINDOW, "-f", str(one)], "at least 2")


def test_through_the_server(tmp_path, sock_dir):
    """`greedy` one-shot and through `dandd serve` + client: the same bytes (the pattern of tests/test_server.py)."""
    env = dict(os.environ, PYTHONHASHSEED="0", SERVER_WORKER_BACKEND="oracle")
    env.pop("DANDD_SERVER", None)
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    out = str(tmp_path / "out")
    os.makedirs(out)

    def one_shot(argv):
        r = subprocess.run([sys.executable, WORKER, "run"] + argv, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (argv, r.stdout[-2000:], r.stderr[-3000:])
    one_shot(["tree", "-d", data, "-o", out, "-s", "t", "-k", "10", "-r", "12", "-c", os.path.join(out, "sketchdb")])
    pk = os.path.join(out, "t_5_dashing_dtree.pickle")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    argv = ["greedy", "-d", pk, *WINDOW, "--steps", "4"]
    one_shot(argv + ["-o", a])
    sock = os.path.join(sock_dir, "dandd.sock")
    srv = subprocess.Popen([sys.executable, WORKER, "serve", sock], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        line = srv.stdout.readline()
        assert "listening" in line, line + srv.stderr.read()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client"] + argv + ["-o", b], env=cenv, capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        bad = subprocess.run([sys.executable, "-m", "dandd_amd.host.client"] + argv + ["-o", b, "--steps", "9"], env=cenv, capture_output=True,
                             text=True, timeout=600, cwd=ROOT)
        assert bad.returncode == 1 and "--steps 9" in bad.stderr
        from dandd_amd.host.client import request
        assert request(sock, {"op": "shutdown"})["rc"] == 0
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
    got, want = _outputs(b), _outputs(a)
    assert len(want) == 4 and got == want
