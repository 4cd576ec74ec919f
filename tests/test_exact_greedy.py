"""`dandd greedy` on an exact tree, on the CPU: the host path only.  A backend's greedy_cards is asked first on every tree;
HipExactBackend answers for 17..64 genomes (dd_exact_greedy) and says None at 16 and below, where the table of all subsets
answers every step.  Here a stand-in gives greedy_cards from Python sets of pyref.kmers, with the same None: at 17 genomes
there is one call per mode and the files are those of the object path (one SubSpider per step and candidate); at 5 the
subset table is still what the walk reads.  The GPU's walk is compared with the same sets in test_gpu_exact_greedy.py."""
import glob
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import pyref
import test_exact_schedules as ex
import test_greedy as tg


class GreedySets(ex.ExactSchedules):
    """ex.ExactSchedules (hostcheck.ExactBackend + the union tables) with greedy_cards: unions of Python sets, walked by
    test_greedy._walk's statement of the rule.  None for n <= 16, as HipExactBackend."""
    name = "exact+greedy"
    greedy_calls = []          # (n, mode) of every greedy_cards call

    def greedy_cards(self, leaf_paths, mode, nfixed, nsteps, kmin):
        type(self).greedy_calls.append((len(leaf_paths), mode))
        if len(leaf_paths) <= 16:
            return None
        dbs = [[json.load(open(p)) for p in row] for row in leaf_paths]
        ks = [int(db["k"]) for db in dbs[0]]
        assert ks == list(range(kmin, kmin + len(ks)))
        for row in dbs:
            assert [int(db["k"]) for db in row] == ks and all(len(db["fastas"]) == 1 for db in row)
        fas = [open(row[0]["fastas"][0], "rb").read() for row in dbs]
        sets = [[set(pyref.kmers(fa, k, self.canonical)) for k in ks] for fa in fas]

        def card_of(chosen, c):
            return [float(len(set().union(*[sets[i][kk] for i in list(chosen) + [c]]))) for kk in range(len(ks))]
        order, cards = tg._walk(card_of, len(fas), nfixed, nsteps, mode, ks)
        return np.array(order), np.array(cards)


class NoGreedy(GreedySets):
    """the entry point, and no walk for these leaves (HipExactBackend whose masks do not fit their store)"""
    name = "exact+nogreedy"

    def greedy_cards(self, leaf_paths, mode, nfixed, nsteps, kmin):
        type(self).greedy_calls.append((len(leaf_paths), mode))


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def _files(d):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(d, "*greedy*"))}


def _tree_of_17(work, host):
    """17 genomes of 90 bp: an ancestor with substitutions, two of them the same bytes"""
    from dandd_amd.host import cli
    data = os.path.join(work, "many")
    os.makedirs(data)
    rng = np.random.default_rng(17)
    anc = rng.integers(0, 4, 90)
    for i in range(17):
        s = anc.copy()
        mut = rng.random(90) < 0.15
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        if i == 11:
            s = last
        last = s
        with open(os.path.join(data, f"t{i:02d}.fasta"), "w") as f:
            f.write(f">t{i}\n" + "".join("ACGT"[c] for c in s) + "\n")
    out = os.path.join(work, "mt")
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", out, "-s", "many", "-k", "8", "--exact"])
    (pk,) = glob.glob(os.path.join(out, "*dtree.pickle"))
    return data, pk


WINDOW = ["--ksweep", "--mink", "7", "--maxk", "9"]


def test_seventeen_genomes_one_call_per_mode_and_the_object_paths_files(host, tmp_path):
    data, pk = _tree_of_17(str(tmp_path), host)
    basef = tmp_path / "base.txt"
    basef.write_text("t05.fasta\n" + os.path.join(data, "t02.fasta") + "\n")
    configs = [(["--mode", "both"], 2), (["--mode", "min", "-b", str(basef), "--steps", "9"], 1)]
    for ci, (extra, nmodes) in enumerate(configs):
        sch, obj, none = (str(tmp_path / f"{name}{ci}") for name in ("sched", "object", "none"))
        GreedySets.reset()
        GreedySets.greedy_calls = []
        ex.run(host, GreedySets, "greedy", [*WINDOW, *extra], pk, sch)
        assert [n for n, _ in GreedySets.greedy_calls] == [17] * nmodes                 # one call per mode ...
        assert len({m for _, m in GreedySets.greedy_calls}) == nmodes
        assert "subset_cards" not in GreedySets.calls                                  # ... no table of 2^17 subsets ...
        assert not [m for m, _ in GreedySets.cards if m >= 2]                          # ... and no union counted on its own
        got = _files(sch)
        # a backend that has no walk for these leaves: asked once per mode, then the object path (first: no union is in the
        # cardinality cache yet)
        NoGreedy.reset()
        NoGreedy.greedy_calls = []
        ex.run(host, NoGreedy, "greedy", [*WINDOW, *extra], pk, none)
        assert len(NoGreedy.greedy_calls) == nmodes and (ci > 0 or any(m >= 2 for m, _ in NoGreedy.cards))
        assert _files(none) == got
        ex.run(host, hostcheck.ExactBackend, "greedy", [*WINDOW, *extra], pk, obj, prefetch=False)
        assert len(got) == 2 + nmodes and got == _files(obj)
    # the twins: t10 stands in front of t11 in the universe, and is taken first
    for mode in ("max", "min"):
        names = [os.path.basename(x) for x in open(glob.glob(os.path.join(str(tmp_path / "sched0"), f"*greedy_{mode}.txt"))[0]).read().split()]
        assert len(names) == 17 and names.index("t10.fasta") < names.index("t11.fasta")


def test_five_genomes_still_walk_the_subset_table(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    tab, obj = str(tmp_path / "table"), str(tmp_path / "object")
    GreedySets.reset()
    GreedySets.greedy_calls = []
    ex.run(host, GreedySets, "greedy", ["--ksweep", "--mink", "8", "--maxk", "12"], pk, tab)
    assert GreedySets.greedy_calls == [(5, "max"), (5, "min")]                          # asked, None ...
    assert GreedySets.calls.get("subset_cards") == 1                                    # ... and one table for both modes
    assert not [(m, k) for m, k in GreedySets.cards if m >= 2 and 8 <= k <= 12]
    ex.run(host, hostcheck.ExactBackend, "greedy", ["--ksweep", "--mink", "8", "--maxk", "12"], pk, obj, prefetch=False)
    assert len(_files(tab)) == 4 and _files(tab) == _files(obj)


def test_binding_and_backend_have_the_entry_points():
    from dandd_amd import engine
    from dandd_amd.host.backend import HipExactBackend
    assert hasattr(engine.Engine, "exact_greedy") and hasattr(engine.Engine, "exact_greedy_device")
    assert "dd_exact_greedy" in engine.EXPORTS and "dd_exact_greedy_device" in engine.EXPORTS
    assert hasattr(HipExactBackend, "greedy_cards")
    assert engine.load_library().dd_abi_version() == 4
