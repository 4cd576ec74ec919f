"""Exact union schedules on the CPU: the subset-sum arithmetic of dd_exact_subsets_from_hist against brute force, and the
host layer on an exact (`tree --exact`) tree -- kij, progressive, deltadelta and abba take the schedule path (one *_cards
table per command, no card() of a union inside the table's window), write what the object path writes, and give the numbers
of tests/golden/ref_exact.json.  The tables here come from a checker backend over the oracle's exact counter; the GPU's are
checked against the same counter in test_gpu_exact_schedules.py."""
import csv
import glob
import io
import json
import os
import pickle
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck

ORDERINGS = {(0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (1, 3, 4, 0, 2)}     # hostcheck.run_scenarios'


# ---- 1. dd_exact_subsets_from_hist ----------------------------------------------------------------------------------
def _brute(hist, n):
    """|union of the genomes in s| with the k-mers as Python sets: k-mer j of mask m is the pair (m, j)"""
    sets = [set() for _ in range(n)]
    for m, c in enumerate(hist):
        for i in range(n):
            if m >> i & 1:
                sets[i].update((m, j) for j in range(int(c)))
    return sets


@pytest.mark.parametrize("n", [1, 2, 5, 10, 16])
def test_subsets_from_hist_matches_brute_force(n):
    from dandd_amd.engine import exact_subsets_from_hist
    rng = np.random.default_rng(100 + n)
    full = (1 << n) - 1
    everywhere = np.zeros(1 << n, dtype=np.uint64)
    everywhere[full] = 12345                                     # every k-mer in every genome
    sparse = np.zeros(1 << n, dtype=np.uint64)
    sparse[rng.integers(1, 1 << n, size=min(40, 1 << n))] = rng.integers(1, 30, size=min(40, 1 << n)).astype(np.uint64)
    dense = rng.integers(0, 4, size=1 << n).astype(np.uint64) if n <= 10 else sparse
    for hist in (np.zeros(1 << n, dtype=np.uint64), everywhere, sparse, dense):
        got = exact_subsets_from_hist(hist, n)
        assert got.dtype == np.uint64 and got.shape == (1 << n,)
        assert got[0] == 0
        sets = _brute(hist, n)
        masks = range(1 << n) if n <= 10 else [full, 1, 1 << (n - 1), full ^ 1] + [int(x) for x in rng.integers(1, full, size=200)]
        for s in masks:
            want = len(set().union(*[sets[i] for i in range(n) if s >> i & 1])) if s else 0
            assert int(got[s]) == want, (n, s)
    # a k-mer in no genome (mask 0) is in no union
    hist = np.zeros(1 << n, dtype=np.uint64)
    hist[0], hist[full] = 7, 3
    assert [int(v) for v in exact_subsets_from_hist(hist, n)[[0, full]]] == [0, 3]


def test_subsets_from_hist_errors():
    from dandd_amd.engine import exact_subsets_from_hist
    with pytest.raises(ValueError):
        exact_subsets_from_hist(np.zeros(8, dtype=np.uint64), 2)
    with pytest.raises(ValueError):
        exact_subsets_from_hist(np.zeros(1 << 17, dtype=np.uint64), 17)


# ---- 2. the host layer on an exact tree ------------------------------------------------------------------------------
class ExactSchedules(hostcheck.ExactBackend):
    """hostcheck.ExactBackend with the four batch entry points, each union counted by the oracle's exact counter."""
    name = "exact+schedules"
    calls = {}            # method -> calls
    cards = []            # (members, k) of every card() call
    windows = []          # (kmin, kmax) of every table

    @classmethod
    def reset(cls):
        cls.calls, cls.cards, cls.windows = {}, [], []

    def card(self, path):
        s = json.load(open(path))
        type(self).cards.append((len(s["fastas"]), int(s["k"])))
        return super().card(path)

    def _window(self, what, leaf_paths):
        cls = type(self)
        cls.calls[what] = cls.calls.get(what, 0) + 1
        dbs = [[json.load(open(p)) for p in row] for row in leaf_paths]
        ks = [int(db["k"]) for db in dbs[0]]
        assert ks == list(range(ks[0], ks[0] + len(ks)))
        for row in dbs:
            assert [int(db["k"]) for db in row] == ks and all(len(db["fastas"]) == 1 for db in row)
        cls.windows.append((ks[0], ks[-1]))
        fas = [np.fromfile(row[0]["fastas"][0], dtype=np.uint8) for row in dbs]
        memo = {}

        def count(members, k):
            key = (frozenset(members), k)
            if key not in memo:
                memo[key] = float(self.orc.exact_count([fas[i] for i in sorted(key[0])], k, self.canonical)) if members else 0.0
            return memo[key]
        return len(fas), ks, count

    def pairwise_cards(self, leaf_paths):
        n, ks, count = self._window("pairwise_cards", leaf_paths)
        return np.array([[[count({i, j}, k) for k in ks] for j in range(n)] for i in range(n)])

    def progressive_cards(self, leaf_paths, orderings):
        n, ks, count = self._window("progressive_cards", leaf_paths)
        return np.array([[[count(list(o)[:j + 1], k) for k in ks] for j in range(n)] for o in orderings])

    def leave_out_cards(self, leaf_paths, group):
        n, ks, count = self._window("leave_out_cards", leaf_paths)
        group = [int(g) for g in group]
        return np.array([[count([i for i in range(n) if group[i] != g], k) for k in ks] for g in range(max(group) + 2)])

    def subset_cards(self, leaf_paths):
        n, ks, count = self._window("subset_cards", leaf_paths)
        return np.array([[count([i for i in range(n) if s >> i & 1], k) for k in ks] for s in range(1 << n)])


class NoSchedules(ExactSchedules):
    """A backend that has the entry points and no schedule for these leaves (HipExactBackend above 64 of them)."""
    name = "exact+none"

    def pairwise_cards(self, leaf_paths):
        self._window("pairwise_cards", leaf_paths)

    def progressive_cards(self, leaf_paths, orderings):
        self._window("progressive_cards", leaf_paths)

    def leave_out_cards(self, leaf_paths, group):
        self._window("leave_out_cards", leaf_paths)

    def subset_cards(self, leaf_paths):
        self._window("subset_cards", leaf_paths)


# command, its arguments, the entry point it must use
COMMANDS = [
    ("kij", ["--jaccard", "--mink", "8", "--maxk", "12"], "pairwise_cards"),
    ("progressive", ["--ksweep", "--mink", "8", "--maxk", "14"], "progressive_cards"),
    ("deltadelta", [], "leave_out_cards"),
    ("deltadelta", ["--ksweep", "--mink", "8", "--maxk", "14"], "leave_out_cards"),
    ("abba", ["--subsets", "--ksweep", "--mink", "8", "--maxk", "16"], "subset_cards"),
]


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def exact_tree(work, host, backend=hostcheck.ExactBackend):
    from dandd_amd.host import cli
    data = os.path.join(work, "data")
    shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    out = os.path.join(work, "t")
    if backend is not None:
        host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", out, "-s", "gold", "-k", "10", "--exact"])
    with open(os.path.join(out, "sketchdb", "gold_5_orderings.pickle"), "wb") as f:
        pickle.dump(set(ORDERINGS), f)
    return os.path.join(out, "gold_5_kmc_dtree.pickle")


def run(host, backend, command, argv, pk, out, prefetch=True):
    from dandd_amd.host import cli
    os.makedirs(out, exist_ok=True)
    if backend is not None:
        host.set_backend_factory(lambda r, c: backend(r, c))
    if prefetch:
        os.environ.pop("DD_NO_PREFETCH", None)
    else:
        os.environ["DD_NO_PREFETCH"] = "1"
    try:
        with redirect_stdout(io.StringIO()):
            cli.main([command, "-d", pk, "-o", out, *argv])
    finally:
        os.environ.pop("DD_NO_PREFETCH", None)


def same_files(a, b):
    """every CSV of directory a equals b's: byte for byte where there is no `command` column (which says how a number was
    obtained and differs between the two paths), else row for row without it"""
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a, "*.csv")))
    assert names and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b, "*.csv")))
    for name in names:
        with open(os.path.join(a, name), newline="") as f:
            header = next(csv.reader(f))
        if "command" in header:
            assert hostcheck.read_rows(os.path.join(a, name)) == hostcheck.read_rows(os.path.join(b, name)), name
        else:
            with open(os.path.join(a, name), "rb") as x, open(os.path.join(b, name), "rb") as y:
                assert x.read() == y.read(), name
    return names


def against_goldens(command, out):
    """kij / progressive rows == ref_exact.json on every key that holds no sketch name or path (the goldens carry the tool
    name `dashing` in those)"""
    with open(os.path.join(hostcheck.GOLD, "ref_exact.json")) as f:
        gold = json.load(f)["scenarios"]
    pairs = {"kij": [("gold_5_kmc.kij.csv", "kij"), ("gold_5_kmc.j.csv", "kij_jaccard_8_12")],
             "progressive": [("gold_progu0_5_kmc.csv", "progressive_ksweep_8_14"),
                             ("gold_progu0_5_kmcsummary.csv", "progressive_ksweep_8_14_summary")]}[command]
    for name, scenario in pairs:
        rows, want = hostcheck.read_rows(os.path.join(out, name)), gold[scenario]
        assert len(rows) == len(want), (name, len(rows), len(want))
        for i, (r, w) in enumerate(zip(rows, want)):
            for key in w:
                if key not in ("sketchloc", "command"):
                    assert hostcheck.same_cell(r.get(key), w[key]), (name, i, key, r.get(key), w[key])


@pytest.mark.parametrize("command,argv,entry", COMMANDS, ids=[f"{c}{'-ksweep' if '--ksweep' in a else ''}" for c, a, _ in COMMANDS])
def test_schedule_path_on_exact_tree(host, tmp_path, command, argv, entry):
    pk = exact_tree(str(tmp_path), host)
    obj, sch = str(tmp_path / "object"), str(tmp_path / "schedule")
    run(host, ExactSchedules, command, argv, pk, obj, prefetch=False)      # (first: nothing of a table is in any cache yet)
    ExactSchedules.reset()
    run(host, ExactSchedules, command, argv, pk, sch)
    # (c) the command asked for its table, and for no card() of a union inside the table's window
    assert ExactSchedules.calls.get(entry, 0) >= 1, ExactSchedules.calls
    lo = min(w[0] for w in ExactSchedules.windows)
    hi = max(w[1] for w in ExactSchedules.windows)
    inside = [(m, k) for m, k in ExactSchedules.cards if m >= 2 and lo <= k <= hi]
    assert not inside, inside
    # (a) the same files as the object path
    same_files(sch, obj)
    # (b) the reference's numbers over an exact counter
    if command in ("kij", "progressive"):
        against_goldens(command, sch)
        against_goldens(command, obj)


@pytest.mark.parametrize("command,argv,entry", COMMANDS, ids=[f"{c}{'-ksweep' if '--ksweep' in a else ''}" for c, a, _ in COMMANDS])
def test_no_table_means_object_path(host, tmp_path, command, argv, entry):
    pk = exact_tree(str(tmp_path), host)
    obj, none = str(tmp_path / "object"), str(tmp_path / "none")
    NoSchedules.reset()
    run(host, NoSchedules, command, argv, pk, none)
    assert NoSchedules.calls.get(entry, 0) >= 1                   # asked, got None ...
    assert any(m >= 2 for m, _ in NoSchedules.cards)              # ... and counted its unions one by one
    run(host, hostcheck.ExactBackend, command, argv, pk, obj, prefetch=False)
    same_files(none, obj)


def test_hill_climb_window_of_an_exact_tree_is_not_capped_at_32(host, tmp_path):
    from dandd_amd.host.compat import load_tree
    pk = exact_tree(str(tmp_path), host)
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    tree = load_tree(pk)
    exp = dict(tree.experiment, ksweep=None)
    lo, hi = tree._table_window(exp)
    assert hi == tree.root_k() + 3 and lo >= 1
    for leaf in tree.leaf_nodes():
        leaf.bestk = 70
    tree.root.bestk = 70
    assert tree._table_window(exp)[1] == 64
