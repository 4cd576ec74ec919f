"""`dandd abba` on the CPU: exact order effects over all n! orderings from the 2^n subset unions.

The schedule path (every subset from one subset_cards table, here a brute-force oracle union per subset) is checked against
the object path (one SubSpider per subset), against all 120 orderings of the five golden FASTAs through `progressive`, and
against `deltadelta`; the pure expectation function against a brute force over all permutations."""
import ast
import csv
import glob
import io
import itertools
import math
import os
import time
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import test_deltadelta as dd

FILES = ["abba", "abba_contrib", "abba_growth", "abba_subsets"]
WINDOW = ["--ksweep", "--mink", "8", "--maxk", "16"]


class SubsetBackend(hostcheck.ScheduleBackend):
    """The schedule backend with subset_cards, brute force: oracle union over each subset, then oracle card."""
    name = "oracle+subsets"
    calls = 0

    def subset_cards(self, leaf_paths):
        SubsetBackend.calls += 1
        slab = self._slab(leaf_paths)
        n, K = len(slab), len(slab[0])
        out = np.zeros((1 << n, K))
        for s in range(1, 1 << n):
            members = [i for i in range(n) if s >> i & 1]
            for kk in range(K):
                out[s, kk] = self.orc.card(self.orc.union(*[slab[i][kk] for i in members]), self.log2m)
        return out


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)


def _abba(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["abba", *argv])


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _out(d, name):
    return os.path.join(d, f"gold_5_dashing.{name}.csv")


@pytest.mark.parametrize("regs", [14, 20])
def test_schedule_path_equals_object_path(host, tmp_path, regs):
    data, pk = dd._tree(str(tmp_path), host, registers=regs)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    before = SubsetBackend.calls
    _abba(host, SubsetBackend, ["-d", pk, "-o", a, "--subsets", *WINDOW])
    assert SubsetBackend.calls == before + 1                 # one table for all 31 subsets
    _abba(host, hostcheck.ScheduleBackend, ["-d", pk, "-o", b, "--subsets", *WINDOW])
    for name in FILES:
        with open(_out(a, name), "rb") as x, open(_out(b, name), "rb") as y:
            assert x.read() == y.read(), name
    assert len(_rows(_out(a, "abba_subsets"))) == 31
    assert len(_rows(_out(a, "abba"))) == 5 * 4 * 6


def _close(got, want, scale):
    return abs(got - want) <= max(1e-12 * abs(want), 1e-9 * scale)


def _check_against_progressive(host, tmp_path, pk, backend, abba_dir, n=5):
    """All n! orderings through `progressive`, then growth, per-step A-before / A-after means and counts and each genome's
    mean / min / max contribution rebuilt from its rows: they must agree with `abba`'s files."""
    from dandd_amd.host import cli
    from dandd_amd.host.deltatree import _window_delta
    p = str(tmp_path / "prog")
    os.makedirs(p, exist_ok=True)
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["progressive", "-d", pk, "-o", p, *WINDOW, "-n", str(math.factorial(n))])
    tables = [_rows(f) for f in sorted(glob.glob(os.path.join(p, "*progu*.csv")))]
    summ = next(t for t in tables if t and "card" in t[0] and "ordering" in t[0])
    res = next(t for t in tables if t and "fastas" in t[0] and "ordering" in t[0])
    cards = {}
    for r in summ:
        cards.setdefault((int(r["ordering"]), int(r["ngen"])), []).append((int(r["kval"]), float(r["card"])))
    prefix = {}
    for r in res:
        cell = r["fastas"]
        prefix[(int(r["ordering"]), int(r["ngen"]))] = ast.literal_eval(cell) if cell.startswith("[") else cell.split("|")
    added = {(o, s): (set(pre) - set(prefix.get((o, s - 1), []))).pop() for (o, s), pre in prefix.items()}
    orders = sorted({o for o, _ in cards})
    assert len(orders) == np.prod(range(1, n + 1))
    delta = {}
    for key, kc in cards.items():
        kc.sort()
        delta[key] = _window_delta([c for _, c in kc], [k for k, _ in kc])[0]
    assert len({tuple(added[(o, s)] for s in range(1, n + 1)) for o in orders}) == len(orders)   # every ordering once
    dU = delta[(orders[0], n)]
    growth = _rows(os.path.join(abba_dir, "gold_5_dashing.abba_growth.csv"))
    for g in growth:
        ng = int(g["ngen"])
        vals = np.array([delta[(o, ng)] for o in orders])
        assert _close(float(g["mean"]), vals.mean(), dU)
        assert _close(float(g["min"]), vals.min(), dU) and _close(float(g["max"]), vals.max(), dU)
    fastas = [r["fasta"] for r in _rows(os.path.join(abba_dir, "gold_5_dashing.abba_contrib.csv"))]
    inc = {f: [] for f in fastas}
    steps = {}                                               # (a, b, s) -> ([before incs], [after incs])
    for o in orders:
        for s in range(1, n + 1):
            b = added[(o, s)]
            d = delta[(o, s)] - (delta[(o, s - 1)] if s > 1 else 0.0)
            inc[b].append(d)
            pre = set(prefix[(o, s)]) - {b}
            for a in fastas:
                if a != b:
                    steps.setdefault((a, b, s), ([], []))[0 if a in pre else 1].append(d)
    for r in _rows(os.path.join(abba_dir, "gold_5_dashing.abba_contrib.csv")):
        v = np.array(inc[r["fasta"]])
        assert _close(float(r["mean_contrib"]), v.mean(), dU)
        assert _close(float(r["min_contrib"]), v.min(), dU) and _close(float(r["max_contrib"]), v.max(), dU)
    for r in _rows(os.path.join(abba_dir, "gold_5_dashing.abba.csv")):
        if r["step"] == "all":
            bef = [x for s in range(1, n + 1) for x in steps[(r["a"], r["b"], s)][0]]
            aft = [x for s in range(1, n + 1) for x in steps[(r["a"], r["b"], s)][1]]
        else:
            bef, aft = steps[(r["a"], r["b"], int(r["step"]))]
        assert int(r["orderings_a_before"]) == len(bef) and int(r["orderings_a_after"]) == len(aft)
        if bef:
            assert _close(float(r["mean_a_before"]), np.mean(bef), dU)
        else:
            assert r["mean_a_before"] == ""
        if aft:
            assert _close(float(r["mean_a_after"]), np.mean(aft), dU)
        else:
            assert r["mean_a_after"] == ""
        if bef and aft:
            assert _close(float(r["abba"]), np.mean(bef) - np.mean(aft), dU)
        else:
            assert r["abba"] == ""


def test_matches_all_orderings_of_progressive(host, tmp_path):
    data, pk = dd._tree(str(tmp_path), host)
    a = str(tmp_path / "a")
    _abba(host, SubsetBackend, ["-d", pk, "-o", a, *WINDOW])
    _check_against_progressive(host, tmp_path, pk, hostcheck.ScheduleBackend, a)


def test_consistency_with_deltadelta_and_leaves(host, tmp_path):
    from dandd_amd.host.compat import load_tree
    from dandd_amd.host.deltatree import _window_delta
    data, pk = dd._tree(str(tmp_path), host)
    a = str(tmp_path / "a")
    _abba(host, SubsetBackend, ["-d", pk, "-o", a, *WINDOW])
    contrib = _rows(_out(a, "abba_contrib"))
    growth = _rows(_out(a, "abba_growth"))
    o = str(tmp_path / "dd")
    host.set_backend_factory(lambda r, c: dd.LeaveOutBackend(r, c))
    from dandd_amd.host import cli
    with redirect_stdout(io.StringIO()):
        cli.main(["deltadelta", "-d", pk, "-o", o, *WINDOW])
    by_fasta = {r["fastas"]: r for r in _rows(os.path.join(o, "gold_5_dashing.deltadelta.csv"))}
    for r in contrib:
        assert float(r["delta_last"]) == float(by_fasta[r["fasta"]]["deltadelta"])
    dU = float(growth[-1]["mean"])
    assert float(growth[-1]["sd"]) == 0.0 and int(growth[-1]["nsubsets"]) == 1
    assert dU == float(by_fasta[contrib[0]["fasta"]]["delta_all"])
    assert abs(sum(float(r["mean_contrib"]) for r in contrib) - dU) <= 1e-12 * dU
    # delta_alone: each leaf's own window delta
    host.set_backend_factory(lambda r, c: hostcheck.OracleBackend(r, c))
    tree = load_tree(pk)
    by_leaf = {leaf.fastas[0]: leaf for leaf in tree.leaf_nodes()}
    for r in contrib:
        leaf = by_leaf[r["fasta"]]
        leaf.node_ksweep(8, 16)
        want = _window_delta([leaf.ksketches[k].card for k in range(8, 17)], list(range(8, 17)))
        assert (float(r["delta_alone"]), int(r["k_alone"])) == want
    # -A / -B: exactly the two pairs, each with its n step rows and the `all` row
    b = str(tmp_path / "b")
    _abba(host, SubsetBackend, ["-d", pk, "-o", b, "-A", "g3.fasta", "-B", os.path.join(data, "g1.fasta"), *WINDOW])
    rows = _rows(_out(b, "abba"))
    assert [(os.path.basename(r["a"]), os.path.basename(r["b"])) for r in rows] == \
        [("g3.fasta", "g1.fasta")] * 6 + [("g1.fasta", "g3.fasta")] * 6
    assert [r["step"] for r in rows[:6]] == ["1", "2", "3", "4", "5", "all"]
    full = {(r["a"], r["b"], r["step"]): r for r in _rows(_out(a, "abba"))}
    for r in rows:
        assert r == full[(r["a"], r["b"], r["step"])]


def test_expectations_brute_force_n6():
    from dandd_amd.host.deltatree import abba_expectations
    n = 6
    rng = np.random.default_rng(6)
    delta = rng.random(1 << n) * 100
    delta[0] = 0.0
    ex = abba_expectations(delta)
    inc = [[] for _ in range(n)]
    steps = {}
    for perm in itertools.permutations(range(n)):
        mask = 0
        for s, b in enumerate(perm, 1):
            d = delta[mask | 1 << b] - delta[mask]
            inc[b].append(d)
            for a in range(n):
                if a != b:
                    steps.setdefault((a, b, s), ([], []))[0 if mask >> a & 1 else 1].append(d)
            mask |= 1 << b
    for g in range(n):
        assert np.isclose(ex["contrib"][g, 0], np.mean(inc[g]), rtol=1e-12)
        assert ex["contrib"][g, 1] == min(inc[g]) and ex["contrib"][g, 2] == max(inc[g])
    for (a, b, s), (bef, aft) in steps.items():
        if bef:
            assert np.isclose(ex["before"][a, b, s - 1], np.mean(bef), rtol=1e-12)
        else:
            assert np.isnan(ex["before"][a, b, s - 1])
        if aft:
            assert np.isclose(ex["after"][a, b, s - 1], np.mean(aft), rtol=1e-12)
        else:
            assert np.isnan(ex["after"][a, b, s - 1])
    for a in range(n):
        for b in range(n):
            if a != b:
                bef = [x for s in range(1, n + 1) for x in steps[(a, b, s)][0]]
                aft = [x for s in range(1, n + 1) for x in steps[(a, b, s)][1]]
                assert np.isclose(ex["before_all"][a, b], np.mean(bef), rtol=1e-12)
                assert np.isclose(ex["after_all"][a, b], np.mean(aft), rtol=1e-12)
    for ng in range(1, n + 1):
        vals = [delta[m] for m in range(1 << n) if bin(m).count("1") == ng]
        assert ex["growth"][ng - 1, 0] == len(vals)
        assert np.isclose(ex["growth"][ng - 1, 1], np.mean(vals), rtol=1e-12)
        assert np.isclose(ex["growth"][ng - 1, 2], np.std(vals), rtol=1e-12)


def test_expectations_n16_fast():
    from dandd_amd.host.deltatree import abba_expectations
    rng = np.random.default_rng(16)
    delta = rng.random(1 << 16)
    delta[0] = 0.0
    abba_expectations(delta)
    t0 = time.perf_counter()
    ex = abba_expectations(delta)
    took = time.perf_counter() - t0
    assert took <= 0.2, took
    assert np.isclose(ex["contrib"][:, 0].sum(), delta[-1], rtol=1e-12)


def test_exact_tree_object_path(host, tmp_path):
    """An --exact tree of four genomes (KMC stand-in) goes through the object path and agrees with `progressive`."""
    from dandd_amd.host import cli
    data = str(tmp_path / "data")
    os.makedirs(data)
    for name in dd.NAMES[:4]:
        with open(os.path.join(hostcheck.GOLD, "fasta", name), "rb") as f, open(os.path.join(data, name), "wb") as g:
            g.write(f.read())
    out = str(tmp_path / "t")
    os.makedirs(out)
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", out, "-s", "gold", "-k", "10", "--exact"])
    pk = glob.glob(os.path.join(out, "*dtree.pickle"))[0]
    a = str(tmp_path / "a")
    _abba(host, hostcheck.ExactBackend, ["-d", pk, "-o", a, *WINDOW])
    for f in glob.glob(os.path.join(a, "*.csv")):
        os.rename(f, os.path.join(a, "gold_5_dashing" + os.path.basename(f)[os.path.basename(f).index(".abba"):]))
    _check_against_progressive(host, tmp_path, pk, hostcheck.ExactBackend, a, n=4)


def test_errors(host, tmp_path):
    data, pk = dd._tree(str(tmp_path), host)

    def fails(argv, text):
        with pytest.raises(SystemExit) as e:
            _abba(host, SubsetBackend, ["-d", pk, "-o", str(tmp_path / "e"), *argv])
        assert text in str(e.value.code), (argv, e.value.code)
    fails([], "a k window is needed")
    fails([*WINDOW, "-A", "g0.fasta"], "go together")
    fails([*WINDOW, "-A", "g0.fasta", "-B", "g0.fasta"], "the same genome")
    fails([*WINDOW, "-A", "g0.fasta", "-B", "nowhere.fasta"], "not a leaf")
    one = tmp_path / "one.txt"
    one.write_text(os.path.join(data, "g2.fasta") + "\n")
    fails([*WINDOW, "-f", str(one)], "at least 2")
    two = tmp_path / "two.txt"
    two.write_text(os.path.join(data, "g2.fasta") + "\n" + os.path.join(data, "g1.fasta") + "\n")
    fails([*WINDOW, "-f", str(two), "-A", "g0.fasta", "-B", "g1.fasta"], "not in the universe")
    # 17 tiny genomes
    many = str(tmp_path / "many")
    os.makedirs(many)
    rng = np.random.default_rng(17)
    for i in range(17):
        with open(os.path.join(many, f"t{i:02d}.fasta"), "w") as f:
            f.write(f">t{i}\n" + "".join(rng.choice(list("ACGT"), size=300)) + "\n")
    out = str(tmp_path / "mt")
    os.makedirs(out)
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: hostcheck.OracleBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", many, "-o", out, "-s", "many", "-k", "10", "-r", "10"])
    pk17 = glob.glob(os.path.join(out, "*dtree.pickle"))[0]
    with pytest.raises(SystemExit) as e:
        _abba(host, SubsetBackend, ["-d", pk17, "-o", str(tmp_path / "e17"), *WINDOW])
    assert "at most 16" in str(e.value.code) and "-f" in str(e.value.code)
