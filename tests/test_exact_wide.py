"""The wide exact union schedules (65 to 255 genomes from one sort per k) without a GPU: the entry points in every layer, the
reference the GPU tests compare against (tests/wide_ref.py) checked against the oracle's exact counter, and the host layer on
an exact tree of 70 tiny genomes -- with a backend that has the wide_ tables `kij`, `progressive` and `deltadelta` ask for them
and count no union on their own, and write what the object path writes; with one that has none they take the object path."""
import io
import json
import os
import pickle
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import test_exact_schedules as cpu
from wide_ref import WideRef

N_TREE = 70
WIDE_NAMES = {"dd_exact_wide_pairwise", "dd_exact_wide_progressive", "dd_exact_wide_leave_out",
              "dd_exact_wide_pairwise_device", "dd_exact_wide_progressive_device", "dd_exact_wide_leave_out_device"}


def tiny_genomes(n, seed, lo=200, hi=300):
    """n genomes of lo..hi bases: one ancestor, 3 % substitutions each, two records, an N and a lowercase stretch"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, hi)
    out = []
    for i in range(n):
        s = anc[:int(rng.integers(lo, hi + 1))].copy()
        mut = rng.random(len(s)) < 0.03
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        t = "".join("ACGT"[c] for c in s)
        a = len(t) // 2 + i % 5
        out.append(f">g{i}_a\n{t[:60]}N{t[60:a].lower()}\n>g{i}_b\n{t[a:]}\n".encode())
    return out


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    assert WIDE_NAMES <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert WIDE_NAMES <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_wide.hip" in build.SOURCES and "dd_exact_runs.h" in build.HEADERS
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in WIDE_NAMES)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert WIDE_NAMES <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    for what in ("pairwise", "progressive", "leave_out"):
        assert hasattr(engine.Engine, f"exact_wide_{what}") and hasattr(engine.Engine, f"exact_wide_{what}_device")
        assert hasattr(HipExactBackend, f"wide_{what}_cards")
    assert HipExactBackend.MAX_WIDE_LEAVES == 255 and HipExactBackend.MAX_LEAVES == 64
    assert "255 genomes" in cli.__doc__
    for command in ("kij", "progressive", "deltadelta"):
        with pytest.raises(SystemExit), redirect_stdout(io.StringIO()) as out:
            cli.build_parser().parse_args([command, "-h"])
        assert "255" in out.getvalue(), command


# ---- 2. the reference against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
def test_reference_matches_the_oracle(orc, canonical):
    n = 67
    fas = tiny_genomes(n, 11)
    fas[5], fas[9], fas[n - 1] = fas[2], b">short\nACGTTGCAT\n", b""
    ref = WideRef(fas, canonical)
    rng = np.random.default_rng(3)
    ords = [list(range(n)), [int(x) for x in rng.permutation(n)]]
    group = [(0, 1, -1)[i % 3] for i in range(n)]
    for k in (5, 11, 31, 33, 64):
        def want(members):
            return orc.exact_count([fas[i] for i in members], k, canonical) if len(members) else 0
        pw, pr, lo = ref.pairwise(k, k), ref.progressive(k, k, ords), ref.leave_out(k, k, group)
        for i, j in [(0, 0), (0, 1), (2, 5), (9, 9), (3, n - 1), (64, 66), (n - 1, n - 1)]:
            assert int(pw[i, j, 0]) == int(pw[j, i, 0]) == want(sorted({i, j})) == ref.count({i, j}, k), (k, i, j)
        for o, j in [(0, 0), (0, 40), (1, 3), (1, 65), (1, n - 1)]:
            assert int(pr[o, j, 0]) == want(sorted(ords[o][:j + 1])) == ref.count(ords[o][:j + 1], k), (k, o, j)
        for g in range(3):
            assert int(lo[g, 0]) == want([i for i in range(n) if group[i] != g]), (k, g)
        assert int(lo[2, 0]) == int(pr[0, n - 1, 0]) == want(list(range(n)))


# ---- 3. the host layer on an exact tree of 70 genomes ---------------------------------------------------------------------
class NarrowOnly(cpu.ExactSchedules):
    """What HipExactBackend was before the wide tables: the three union tables, and None for more than 64 leaves."""
    name = "exact+narrow"

    def _narrow(self, what, leaf_paths, *args):
        if len(leaf_paths) > 64:
            self._window(what, leaf_paths)
            return None
        return getattr(super(), what)(leaf_paths, *args)

    def pairwise_cards(self, leaf_paths):
        return self._narrow("pairwise_cards", leaf_paths)

    def progressive_cards(self, leaf_paths, orderings):
        return self._narrow("progressive_cards", leaf_paths, orderings)

    def leave_out_cards(self, leaf_paths, group):
        return self._narrow("leave_out_cards", leaf_paths, group)


class WideChecker(NarrowOnly):
    """... and with the three wide_ tables, each from tests/wide_ref.py"""
    name = "exact+wide"

    def _ref(self, what, leaf_paths):
        cls = type(self)
        cls.calls[what] = cls.calls.get(what, 0) + 1
        dbs = [[json.load(open(p)) for p in row] for row in leaf_paths]
        ks = [int(db["k"]) for db in dbs[0]]
        assert ks == list(range(ks[0], ks[0] + len(ks))) and len(dbs) <= 255
        cls.windows.append((ks[0], ks[-1]))
        return WideRef([open(row[0]["fastas"][0], "rb").read() for row in dbs], self.canonical), ks[0], ks[-1]

    def wide_pairwise_cards(self, leaf_paths):
        ref, kmin, kmax = self._ref("wide_pairwise_cards", leaf_paths)
        return ref.pairwise(kmin, kmax).astype(np.float64)

    def wide_progressive_cards(self, leaf_paths, orderings):
        ref, kmin, kmax = self._ref("wide_progressive_cards", leaf_paths)
        return ref.progressive(kmin, kmax, orderings).astype(np.float64)

    def wide_leave_out_cards(self, leaf_paths, group):
        ref, kmin, kmax = self._ref("wide_leave_out_cards", leaf_paths)
        return ref.leave_out(kmin, kmax, group).astype(np.float64)


def wide_tree(work, host, backend, n=N_TREE):
    """an exact tree of n tiny genomes -> (its pickle, the list of four FASTAs `deltadelta -f` leaves out)"""
    from dandd_amd.host import cli
    data = os.path.join(work, "data")
    os.makedirs(data)
    files = []
    for i, fa in enumerate(tiny_genomes(n, 70)):
        files.append(os.path.join(data, f"w{i:03d}.fa"))
        with open(files[-1], "wb") as f:
            f.write(fa)
    out = os.path.join(work, "t")
    if backend is not None:
        host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", out, "-s", "wide", "-k", "10", "--exact"])
    rng = np.random.default_rng(n)
    with open(os.path.join(out, "sketchdb", f"wide_{n}_orderings.pickle"), "wb") as f:
        pickle.dump({tuple(int(x) for x in rng.permutation(n)) for _ in range(3)}, f)
    left_out = os.path.join(work, "left_out.txt")
    with open(left_out, "w") as f:
        f.write("".join(files[i] + "\n" for i in (0, 33, 64, n - 1)))
    return os.path.join(out, f"wide_{n}_kmc_dtree.pickle"), left_out


def wide_commands(left_out):
    """command, its arguments, the wide table it must ask for"""
    return [("kij", ["--jaccard", "--mink", "9", "--maxk", "10"], "wide_pairwise_cards"),
            ("progressive", ["-n", "3", "--ksweep", "--mink", "9", "--maxk", "10"], "wide_progressive_cards"),
            ("deltadelta", ["-f", left_out, "--ksweep", "--mink", "9", "--maxk", "10"], "wide_leave_out_cards")]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["kij", "progressive", "deltadelta"])
def test_wide_tables_on_a_tree_of_70(cpu_host, tmp_path, which):
    pk, left_out = wide_tree(str(tmp_path), cpu_host, hostcheck.ExactBackend)
    command, argv, entry = wide_commands(left_out)[which]
    obj, wide = str(tmp_path / "object"), str(tmp_path / "wide")
    cpu.run(cpu_host, hostcheck.ExactBackend, command, argv, pk, obj, prefetch=False)   # (first: nothing is in any cache yet)
    WideChecker.reset()
    cpu.run(cpu_host, WideChecker, command, argv, pk, wide)
    # the command asked the narrow table, got None, asked the wide one, and counted no union of the window on its own
    assert WideChecker.calls.get(entry, 0) >= 1 and WideChecker.calls.get(entry[len("wide_"):], 0) >= 1, WideChecker.calls
    lo = min(w[0] for w in WideChecker.windows)
    hi = max(w[1] for w in WideChecker.windows)
    inside = [(m, k) for m, k in WideChecker.cards if m >= 2 and lo <= k <= hi]
    assert not inside, inside
    cpu.same_files(wide, obj)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["kij", "progressive", "deltadelta"])
def test_no_wide_table_means_object_path(cpu_host, tmp_path, which):
    pk, left_out = wide_tree(str(tmp_path), cpu_host, hostcheck.ExactBackend)
    command, argv, entry = wide_commands(left_out)[which]
    obj, none = str(tmp_path / "object"), str(tmp_path / "none")
    NarrowOnly.reset()
    cpu.run(cpu_host, NarrowOnly, command, argv, pk, none)
    assert NarrowOnly.calls.get(entry[len("wide_"):], 0) >= 1                  # asked, got None ...
    assert any(m >= 2 for m, _ in NarrowOnly.cards)                            # ... and counted its unions one by one
    cpu.run(cpu_host, hostcheck.ExactBackend, command, argv, pk, obj, prefetch=False)
    cpu.same_files(none, obj)


def test_safe_and_no_prefetch_keep_the_object_path(cpu_host, tmp_path):
    pk, left_out = wide_tree(str(tmp_path), cpu_host, hostcheck.ExactBackend)
    command, argv, entry = wide_commands(left_out)[1]
    for tag, extra, prefetch in (("safe", ["--safe"], True), ("noprefetch", [], False)):
        WideChecker.reset()
        cpu.run(cpu_host, WideChecker, command, argv + extra, pk, str(tmp_path / tag), prefetch=prefetch)
        assert not WideChecker.calls, (tag, WideChecker.calls)


@pytest.fixture
def cpu_host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)
