"""`dandd core` on the CPU: the k-mer spectrum, the core of every prefix of an ordering next to its union, and the core,
private k-mers and signature of groups, on the golden exact tree.  The three tables come from a checker backend that builds
the membership masks from Python sets of pyref.kmers; every cell of every file is compared with the same sets, the `pan`
column with what `progressive` writes, and the command's exits are checked.  The GPU's tables are compared with the same
masks in test_gpu_core.py."""
import csv
import glob
import io
import json
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import pyref
import test_exact_schedules as ex

WINDOW = ["--ksweep", "--mink", "8", "--maxk", "12"]
KS = list(range(8, 13))
NAMES = ["g0.fasta", "g1.fasta", "g2.fasta", "g3.fasta", "g4.fasta"]
ORDERINGS = sorted(ex.ORDERINGS)


def masks_of(fas, k, canonical=True):
    """{k-mer: membership mask} over the FASTA buffers `fas` (bit i: fas[i] holds it)"""
    out = {}
    for i, fa in enumerate(fas):
        for x in set(pyref.kmers(fa, k, canonical)):
            out[x] = out.get(x, 0) | 1 << i
    return out


def spectrum_of(masks, n):
    spec = [0] * (n + 1)
    for m in masks.values():
        spec[bin(m).count("1")] += 1
    return spec


def select_of(masks, al, no):
    return sum(1 for m in masks.values() if m & al == al and m & no == 0)


def core_of(masks, order):
    """[j] = k-mers held by every one of order[0..j]"""
    out, need = [], 0
    for g in order:
        need |= 1 << g
        out.append(select_of(masks, need, 0))
    return out


class CoreBackend(hostcheck.ExactBackend):
    """hostcheck.ExactBackend with the three intersection tables, from Python sets."""
    name = "exact+core"
    calls = {}

    @classmethod
    def reset(cls):
        cls.calls = {}

    def _masks(self, what, leaf_paths):
        cls = type(self)
        cls.calls[what] = cls.calls.get(what, 0) + 1
        dbs = [[json.load(open(p)) for p in row] for row in leaf_paths]
        ks = [int(db["k"]) for db in dbs[0]]
        assert ks == list(range(ks[0], ks[0] + len(ks)))
        for row in dbs:
            assert [int(db["k"]) for db in row] == ks and all(len(db["fastas"]) == 1 for db in row)
        fas = [open(row[0]["fastas"][0], "rb").read() for row in dbs]
        return len(fas), [masks_of(fas, k, self.canonical) for k in ks]

    def spectrum_counts(self, leaf_paths):
        n, per_k = self._masks("spectrum_counts", leaf_paths)
        return np.array([spectrum_of(m, n) for m in per_k], dtype=np.uint64).T

    def core_progressive_counts(self, leaf_paths, orderings):
        n, per_k = self._masks("core_progressive_counts", leaf_paths)
        return np.array([[core_of(m, o) for m in per_k] for o in orderings], dtype=np.uint64).transpose(0, 2, 1)

    def select_counts(self, leaf_paths, all_masks, none_masks):
        n, per_k = self._masks("select_counts", leaf_paths)
        return np.array([[select_of(m, int(a), int(b)) for m in per_k] for a, b in zip(all_masks, none_masks)], dtype=np.uint64)


class CoreAndProgressive(CoreBackend):
    """... and the union table `progressive` uses on the GPU: `pan` then comes from one progressive_cards call."""
    name = "exact+core+progressive"

    def progressive_cards(self, leaf_paths, orderings):
        n, per_k = self._masks("progressive_cards", leaf_paths)
        return np.array([[[float(sum(1 for m in masks.values() if m & sum(1 << g for g in o[:j + 1]))) for masks in per_k]
                          for j in range(n)] for o in orderings])


class NoMasks(CoreBackend):
    """the entry points, and no table for these leaves (HipExactBackend above 64 of them)"""
    name = "exact+nomasks"

    def spectrum_counts(self, leaf_paths):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def _core(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["core", *argv])


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _outputs(d):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(d, "*.core_*"))}


def _delta(cards, ks):
    """the rule of `abba` and `greedy`, written out on its own: largest card / k, a later k winning a tie"""
    best, bestk = 0, 0
    for c, k in zip(cards, ks):
        if c / k >= best:
            best, bestk = c / k, k
    return best, bestk


def _golden(data, names=NAMES):
    fas = [open(os.path.join(data, n), "rb").read() for n in names]
    return {k: masks_of(fas, k) for k in KS}


def _groups_file(tmp_path, data):
    g = tmp_path / "groups.tsv"
    g.write_text(f"{os.path.join(data, 'g0.fasta')}\tleft\ng3.fasta\tright\n{os.path.join(data, 'g2.fasta')}\tleft\ng4.fasta\tright\n"
                 "g1.fasta\talone\n")
    return str(g), [("left", [0, 2]), ("right", [3, 4]), ("alone", [1])]


def test_every_cell_equals_the_set_computation(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = _groups_file(tmp_path, data)
    pickle_path = os.path.join(str(tmp_path), "t", "sketchdb", "gold_5_orderings.pickle")
    out = str(tmp_path / "o")
    CoreBackend.reset()
    _core(host, CoreBackend, ["-d", pk, "-o", out, "-r", pickle_path, "-g", gfile, *WINDOW])
    assert CoreBackend.calls == {"spectrum_counts": 1, "core_progressive_counts": 1, "select_counts": 1}
    prefix = os.path.join(out, "gold_5_kmc")
    assert sorted(_outputs(out)) == sorted(f"gold_5_kmc.core_{x}.csv" for x in ("spectrum", "growth", "growthsummary", "groups", "groupsummary"))
    want = _golden(data)
    fastas = [os.path.join(data, n) for n in NAMES]
    # spectrum
    rows = _rows(prefix + ".core_spectrum.csv")
    assert list(rows[0]) == ["k", "ngen", "kmers"]
    assert [(int(r["k"]), int(r["ngen"])) for r in rows] == [(k, j) for k in KS for j in range(1, 6)]
    for r in rows:
        assert int(r["kmers"]) == spectrum_of(want[int(r["k"])], 5)[int(r["ngen"])], r
    # growth: the orderings in the order the pickle's set lists them
    import pickle
    with open(pickle_path, "rb") as f:
        orderings = list(pickle.load(f))
    assert sorted(orderings) == ORDERINGS
    rows = _rows(prefix + ".core_growth.csv")
    assert list(rows[0]) == ["ordering", "step", "fasta", "k", "pan", "core"]
    assert len(rows) == 3 * 5 * len(KS)
    it = iter(rows)
    curves = {}
    for o, order in enumerate(orderings):
        for j, g in enumerate(order):
            need = sum(1 << x for x in order[:j + 1])
            for k in KS:
                r = next(it)
                assert (int(r["ordering"]), int(r["step"]), r["fasta"], int(r["k"])) == (o + 1, j + 1, fastas[g], k)
                assert int(r["core"]) == select_of(want[k], need, 0), r
                assert int(r["pan"]) == len(want[k]) - select_of(want[k], 0, need), r
                curves.setdefault((o + 1, j + 1), ([], []))
                curves[(o + 1, j + 1)][0].append(int(r["pan"]))
                curves[(o + 1, j + 1)][1].append(int(r["core"]))
        assert curves[(o + 1, 5)][1] == [spectrum_of(want[k], 5)[5] for k in KS]          # the core of all = spectrum[n]
    rows = _rows(prefix + ".core_growthsummary.csv")
    assert list(rows[0]) == ["ordering", "step", "fasta", "pan_delta", "pan_k", "core_delta", "core_k"]
    assert len(rows) == 15
    for r in rows:
        pan, core = curves[(int(r["ordering"]), int(r["step"]))]
        assert (float(r["pan_delta"]), int(r["pan_k"])) == _delta(pan, KS)
        assert (float(r["core_delta"]), int(r["core_k"])) == _delta(core, KS)
        assert r["fasta"] == fastas[orderings[int(r["ordering"]) - 1][int(r["step"]) - 1]]
    # groups
    rows = _rows(prefix + ".core_groups.csv")
    assert list(rows[0]) == ["group", "ngen", "k", "core", "private", "signature"]
    assert [(r["group"], int(r["k"])) for r in rows] == [(label, k) for label, _ in groups for k in KS]
    cols = {}
    for r in rows:
        members = dict(groups)[r["group"]]
        G = sum(1 << i for i in members)
        k = int(r["k"])
        assert int(r["ngen"]) == len(members)
        assert int(r["core"]) == select_of(want[k], G, 0)
        assert int(r["private"]) == select_of(want[k], 0, 31 ^ G)
        assert int(r["signature"]) == select_of(want[k], G, 31 ^ G)
        assert int(r["signature"]) <= min(int(r["core"]), int(r["private"]))
        for c in ("core", "private", "signature"):
            cols.setdefault((r["group"], c), []).append(int(r[c]))
    rows = _rows(prefix + ".core_groupsummary.csv")
    assert [r["group"] for r in rows] == [label for label, _ in groups]
    for r in rows:
        for c in ("core", "private", "signature"):
            assert (float(r[f"{c}_delta"]), int(r[f"{c}_k"])) == _delta(cols[(r["group"], c)], KS), (r, c)
    # a single genome's private k-mers and signature are the same thing
    assert cols[("alone", "private")] == cols[("alone", "signature")]


def test_pan_column_equals_progressive(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    pickle_path = os.path.join(str(tmp_path), "t", "sketchdb", "gold_5_orderings.pickle")
    a, b, p = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "p")
    _core(host, CoreBackend, ["-d", pk, "-o", a, "-r", pickle_path, *WINDOW])           # pan: one SubSpider per prefix
    CoreAndProgressive.reset()
    _core(host, CoreAndProgressive, ["-d", pk, "-o", b, "-r", pickle_path, *WINDOW])    # pan: one progressive_cards table
    assert CoreAndProgressive.calls == {"spectrum_counts": 1, "core_progressive_counts": 1, "progressive_cards": 1}
    assert _outputs(a) == _outputs(b) and len(_outputs(a)) == 3
    ex.run(host, hostcheck.ExactBackend, "progressive", WINDOW, pk, p)
    summ = _rows(os.path.join(p, "gold_progu0_5_kmcsummary.csv"))
    want = {(int(r["ordering"]), int(r["ngen"]), int(r["kval"])): float(r["card"]) for r in summ}
    rows = _rows(os.path.join(a, "gold_5_kmc.core_growth.csv"))
    assert len(rows) == len(want) == 3 * 5 * len(KS)
    for r in rows:
        assert float(r["pan"]) == want[(int(r["ordering"]), int(r["step"]), int(r["k"]))], r


def test_default_ordering_universe_and_window(host, tmp_path):
    """no -r / -n: one ordering, the genomes as listed by -f; the window of a tree built with --ksweep needs no flags"""
    from dandd_amd.host import cli
    data = str(tmp_path / "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    t = str(tmp_path / "t")
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", t, "-s", "gold", "--exact", *WINDOW])
    pk = os.path.join(t, "gold_5_kmc_dtree.pickle")
    names = ["g3.fasta", "g0.fasta", "g4.fasta"]
    flist = tmp_path / "three.txt"
    flist.write_text("".join(os.path.join(data, n) + "\n" for n in names))
    gfile = tmp_path / "g.tsv"
    gfile.write_text("g4.fasta\tx\ng3.fasta\tx\n")
    out = str(tmp_path / "o")
    _core(host, CoreBackend, ["-d", pk, "-o", out, "-f", str(flist), "-g", str(gfile), "-l", "lab"])
    want = _golden(data, names)
    prefix = os.path.join(out, "gold_lab_5_kmc")
    rows = _rows(prefix + ".core_spectrum.csv")
    assert [(int(r["k"]), int(r["ngen"])) for r in rows] == [(k, j) for k in KS for j in (1, 2, 3)]
    assert all(int(r["kmers"]) == spectrum_of(want[int(r["k"])], 3)[int(r["ngen"])] for r in rows)
    rows = _rows(prefix + ".core_growth.csv")
    assert [os.path.basename(r["fasta"]) for r in rows[::len(KS)]] == names and {r["ordering"] for r in rows} == {"1"}
    for r in rows:
        need = (1 << int(r["step"])) - 1
        assert int(r["core"]) == select_of(want[int(r["k"])], need, 0)
    rows = _rows(prefix + ".core_groups.csv")
    for r in rows:                                                    # x = {g4, g3} = bits 2 and 0 of the universe of three
        assert (int(r["core"]), int(r["private"]), int(r["signature"])) == \
            (select_of(want[int(r["k"])], 5, 0), select_of(want[int(r["k"])], 0, 2), select_of(want[int(r["k"])], 5, 2))
    # a group member outside the universe
    bad = tmp_path / "bad.tsv"
    bad.write_text("g1.fasta\tx\n")
    with pytest.raises(SystemExit) as e:
        _core(host, CoreBackend, ["-d", pk, "-o", out, "-f", str(flist), "-g", str(bad)])
    assert "not in the universe" in str(e.value.code)


def test_exits(host, tmp_path):
    import test_deltadelta as dd
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            _core(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("core: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*.core_*"))
    fails(CoreBackend, ["-d", pk], "a k window is needed")
    # -g as in deltadelta: a malformed line, a name that is no leaf
    bad = tmp_path / "bad.tsv"
    bad.write_text("g0.fasta one\n")
    fails(CoreBackend, ["-d", pk, *WINDOW, "-g", str(bad)], "expected 'fasta<TAB>group'", "bad.tsv:1")
    bad.write_text("nowhere.fasta\tone\n")
    fails(CoreBackend, ["-d", pk, *WINDOW, "-g", str(bad)], "not a leaf")
    empty = tmp_path / "empty.txt"
    empty.write_text("nowhere.fasta\n")
    fails(CoreBackend, ["-d", pk, *WINDOW, "-f", str(empty)], "0 genomes", "at least 1")
    fails(NoMasks, ["-d", pk, *WINDOW], "no membership masks")
    fails(hostcheck.ExactBackend, ["-d", pk, *WINDOW], "spectrum_counts")
    # a tree of sketches
    sk = tmp_path / "sk"
    sk.mkdir()
    _, pks = dd._tree(str(sk), host)
    fails(CoreBackend, ["-d", pks, *WINDOW], "tree --exact", "inclusion-exclusion")
    # 65 tiny genomes
    many = str(tmp_path / "many")
    os.makedirs(many)
    rng = np.random.default_rng(65)
    for i in range(65):
        with open(os.path.join(many, f"t{i:02d}.fasta"), "w") as f:
            f.write(f">t{i}\n" + "".join(rng.choice(list("ACGT"), size=60)) + "\n")
    out = str(tmp_path / "mt")
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", many, "-o", out, "-s", "many", "-k", "10", "--exact"])
    pk65 = glob.glob(os.path.join(out, "*dtree.pickle"))[0]
    fails(CoreBackend, ["-d", pk65, *WINDOW], "65 genomes", "at most 64", "-f")


def test_group_queries_in_class_order(host):
    """The one table of the k-mer classes: core (G, 0), private (0, full ^ G), signature (G, full ^ G), group after group"""
    full = 0b111
    assert host.group_queries([0b011, 0b100], full) == ([3, 0, 3, 4, 0, 4], [0, 4, 4, 0, 3, 3])
    assert host.DeltaTree.KMER_CLASSES == tuple(host.KMER_QUERIES) == ("core", "private", "signature")
    for G in (0b011, 0b100):
        alls, nones = host.group_queries([G], full)
        assert list(zip(alls, nones)) == [host.KMER_QUERIES[cls](G, full) for cls in host.DeltaTree.KMER_CLASSES]
    assert host.group_queries([], full) == ([], [])


def test_universe_of_a_call(host, tmp_path, monkeypatch):
    """DeltaTree._universe on the golden exact tree: the window's checks, leaf files only when asked for, the object path of
    one union, and the backend's two failures."""
    from dandd_amd.host.compat import load_tree
    pk = ex.exact_tree(str(tmp_path), host)                       # (leaves hostcheck.ExactBackend as the backend)
    data = str(tmp_path / "data")
    tree = load_tree(pk)
    fastas = [os.path.join(data, n) for n in NAMES[1:4]]
    with pytest.raises(ValueError, match=r"^empty k window 9\.\.8$"):
        tree._universe(fastas, 9, 8)
    with pytest.raises(ValueError, match=r"^empty k window 1\.\.0$"):
        tree._universe(fastas, -3, 0)
    passes = []
    leaf_files = host.DeltaTree._leaf_files
    monkeypatch.setattr(host.DeltaTree, "_leaf_files", lambda self, nodes, lo, hi: passes.append((len(nodes), lo, hi)) or leaf_files(self, nodes, lo, hi))
    u = tree._universe(fastas, 8, 10)
    assert (u.n, u.full, u.lo, u.hi, u.ks) == (3, 0b111, 8, 10, [8, 9, 10])
    assert u.index == {f: i for i, f in enumerate(fastas)} and [leaf.fastas[0] for leaf in u.nodes] == fastas
    assert u.exp["ksweep"] == (8, 10) and tree.experiment["ksweep"] is None and u.batched
    assert tree._universe(fastas, 0, 2).ks == [1, 2]
    assert u.masks([[fastas[2]], [fastas[1], fastas[0], fastas[1]]]) == [0b100, 0b011]
    cards = u.union_cards([0, 2])
    assert passes == []                                           # the object path never asks for the leaves' files
    sub = host.SubSpider([u.nodes[0], u.nodes[2]], tree.speciesinfo, u.exp)
    sub.root.node_ksweep(8, 10)
    assert cards == [sub.root.ksketches[k].card for k in (8, 9, 10)]
    texts = [open(fastas[i], "rb").read() for i in (0, 2)]
    assert cards == [float(pyref.exact_count(texts, k, True)) for k in (8, 9, 10)]
    paths = u.paths
    assert u.paths is paths and passes == [(3, 8, 10)]
    assert [[int(json.load(open(p))["k"]) for p in row] for row in paths] == [[8, 9, 10]] * 3
    u.need("leaf", "card", why="intersections need")
    with pytest.raises(ValueError, match="^the backend exact has no spectrum_counts: intersections need exact membership masks$"):
        u.need("leaf", "spectrum_counts", "select_counts", why="intersections need")
    with pytest.raises(ValueError, match="^the backend exact has no screen_counts: containment needs exact membership masks$"):
        u.need("screen_counts", why="containment needs")
    with pytest.raises(ValueError, match="^the backend has no membership masks for 3 genomes$"):
        u.table(None, (1, 3))
    got = u.table([[1.0, 2.0, 3.0]], (3, 1))
    assert got.dtype == np.uint64 and got.tolist() == [[1], [2], [3]] and u.table((1, 2)) == (1, 2)
    monkeypatch.setenv("DD_NO_PREFETCH", "1")
    assert not tree._universe(fastas, 8, 10).batched
    monkeypatch.delenv("DD_NO_PREFETCH")
    tree.experiment["safety"] = True
    assert not tree._universe(fastas, 8, 10).batched
    # a local of the call: nothing of it stays on the tree, which is pickled
    assert not any(isinstance(v, host._Universe) for v in vars(tree).values())


def test_rank_zero_finishes_alone(host, monkeypatch):
    """abba and greedy under several ranks: every rank presketches the window, and the rank is read BEFORE the barrier at the
    end of presketch_range switches the sharding off (after it every rank reads as rank 0 of 1)."""
    from dandd_amd.host import cli

    class Tree:
        def presketch_range(self, lo, hi):
            swept.append((lo, hi))
            monkeypatch.setattr(host, "dist_ranks", lambda: (0, 1))
    for ranks, alone, sweeps in (((0, 1), True, []), ((0, 2), True, [(8, 12)]), ((1, 2), False, [(8, 12)])):
        swept = []
        monkeypatch.setattr(host, "dist_ranks", lambda ranks=ranks: ranks)
        assert cli._rank0_after_presketch(Tree(), (8, 12)) is alone and swept == sweeps


def test_binding_and_backend_have_the_entry_points():
    from dandd_amd import engine
    from dandd_amd.host.backend import HipExactBackend
    for what in ("spectrum", "core_progressive", "select"):
        assert hasattr(engine.Engine, f"exact_{what}") and hasattr(engine.Engine, f"exact_{what}_device")
        assert f"dd_exact_{what}" in engine.EXPORTS and f"dd_exact_{what}_device" in engine.EXPORTS
    for what in ("spectrum_counts", "core_progressive_counts", "select_counts"):
        assert hasattr(HipExactBackend, what)
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4
