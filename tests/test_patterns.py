"""`dandd patterns` on the CPU: the entry points of every layer, and the command on the golden exact tree with a checker backend
whose pattern_counts comes from Python sets (test_screen.ScreenBackend plus pattern_counts): the three CSVs against tables
computed here from the files' text alone -- the order with its ties, --top and what the summary says of the rows left out,
the arithmetic of --splits -- and the command's exits.  The GPU's table is compared with collections.Counter over
test_core_regions.reference, the 7-input fixture's masks, in test_gpu_patterns.py."""
import collections
import csv
import glob
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as ex
import test_screen as cpus

COLS = {
    "patterns": ["k", "rank", "kmers", "fraction", "ngenomes", "mask", "members"],
    "patterns_summary": ["k", "distinct_kmers", "patterns", "rows_written", "kmers_in_rows", "core", "singletons", "top_members"],
    "splits": ["k", "side_a", "side_b", "support"],
}


def ordered(counter):
    """a Counter over masks -> [(mask, count)], count descending, ties by mask ascending: the order of every layer"""
    return sorted(counter.items(), key=lambda r: (-r[1], r[0]))


def table_of(masks, limit=None):
    """{k-mer: mask} -> what pattern_counts returns"""
    rows = ordered(collections.Counter(masks.values()))
    shown = rows if limit is None else rows[:limit]
    return (np.array([m for m, _ in shown], dtype=np.uint64), np.array([c for _, c in shown], dtype=np.uint64), len(rows), len(masks))


class PatternBackend(cpus.ScreenBackend):
    """test_screen.ScreenBackend with pattern_counts from Python sets."""
    name = "exact+core+regions+screen+patterns"

    def pattern_counts(self, leaf_paths, k, limit):
        import json
        n, per_k = self._masks("pattern_counts", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        return table_of(per_k[0], limit)


class NoPatternMasks(PatternBackend):
    name = "exact+nopatterns"

    def pattern_counts(self, leaf_paths, k, limit):
        return None


def tables(universe, ks, top=1000, splits=False, canonical=True):
    """The files of `patterns` as lists of rows of strings, from sets of pyref.kmers over the texts alone.
    universe: [(name as the CSV shows it, FASTA bytes)]"""
    n = len(universe)
    full = (1 << n) - 1

    def members(mask):
        return ";".join(name for i, (name, _) in enumerate(universe) if mask >> i & 1)
    rows, summary, parts = [], [], []
    for k in ks:
        mask = {}
        for i, (_, fa) in enumerate(universe):
            for x in set(pyref.kmers(fa, k, canonical)):
                mask[x] = mask.get(x, 0) | 1 << i
        count = collections.Counter(mask.values())
        table = ordered(count)
        shown = table[:top] if top else table
        for rank, (m, c) in enumerate(shown, 1):
            rows.append([k, rank, c, c / len(mask), bin(m).count("1"), f"{m:x}", members(m)])
        summary.append([k, len(mask), len(table), len(shown), sum(c for _, c in shown), count.get(full, 0),
                        sum(count.get(1 << i, 0) for i in range(n)), members(shown[0][0])])
        if splits:
            sides = {min(m, full ^ m) for m in count if 2 <= bin(m).count("1") <= n - 2}
            for a in sorted(sides, key=lambda a: (-(count.get(a, 0) + count.get(full ^ a, 0)), a)):
                parts.append([k, members(a), members(full ^ a), count.get(a, 0) + count.get(full ^ a, 0)])
    out = {"patterns": rows, "patterns_summary": summary}
    if splits:
        out["splits"] = parts
    return {name: [[cpus.cell(v) for v in r] for r in body] for name, body in out.items()}


def read_csvs(outdir, prefix="gold_5_kmc"):
    got = {}
    for name in COLS:
        path = os.path.join(outdir, f"{prefix}.{name}.csv")
        if os.path.exists(path):
            with open(path, newline="") as f:
                body = list(csv.reader(f))
            assert body[0] == COLS[name], name
            got[name] = body[1:]
    return got


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def _patterns(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["patterns", *argv])


def golden_universe(data):
    return [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    universe = golden_universe(data)
    ks = [6, 9, 12]
    out = str(tmp_path / "o")
    PatternBackend.reset()
    _patterns(host, PatternBackend, ["-d", pk, "-k", "12", "-k", "6", "-k", "9", "-o", out, "--splits"])
    assert PatternBackend.calls == {"pattern_counts": len(ks)}              # once per k
    want = tables(universe, ks, splits=True)
    got = read_csvs(out)
    assert sorted(got) == ["patterns", "patterns_summary", "splits"]
    for name in want:
        assert got[name] == want[name], name
    # the order, said once more on the file itself: kmers descending, equal kmers by the mask as a number; and ties do occur
    ties = 0
    for k in ks:
        rows = [(int(r[2]), int(r[5], 16)) for r in got["patterns"] if int(r[0]) == k]
        assert rows == sorted(rows, key=lambda r: (-r[0], r[1])) and [int(r[1]) for r in got["patterns"] if int(r[0]) == k] == list(range(1, len(rows) + 1))
        ties += sum(1 for a, b in zip(rows, rows[1:]) if a[0] == b[0])
        s = next(r for r in got["patterns_summary"] if int(r[0]) == k)
        assert int(s[1]) == sum(c for c, _ in rows) == int(s[4]) and int(s[2]) == int(s[3]) == len(rows)
    assert ties > 0
    # the splits: each side's k-mers added, both sides at least two genomes, every bipartition once
    for r in got["splits"]:
        a, b = r[1].split(";"), r[2].split(";")
        assert len(a) >= 2 and len(b) >= 2 and sorted(a + b) == sorted(name for name, _ in universe)
    assert len({(r[0], r[1]) for r in got["splits"]}) == len(got["splits"]) > 0
    # --top: the first rows of the same table; the summary says what they hold, core and singletons stay those of the whole table
    out2 = str(tmp_path / "o2")
    _patterns(host, PatternBackend, ["-d", pk, "-k", "9", "-o", out2, "--top", "3"])
    got2 = read_csvs(out2)
    assert sorted(got2) == ["patterns", "patterns_summary"]
    assert got2 == tables(universe, [9], top=3)
    assert got2["patterns"] == [r for r in got["patterns"] if r[0] == "9"][:3]
    s9 = next(r for r in got["patterns_summary"] if r[0] == "9")
    assert got2["patterns_summary"][0][:3] == s9[:3] and got2["patterns_summary"][0][3] == "3" and got2["patterns_summary"][0][5:7] == s9[5:7]
    assert int(got2["patterns_summary"][0][4]) == sum(int(r[2]) for r in got2["patterns"]) < int(s9[4])
    # --top 0: all; the default k is the root's; -f narrows the universe and renumbers the bits
    out3 = str(tmp_path / "o3")
    flist = tmp_path / "f.txt"
    flist.write_text("".join(os.path.join(data, name) + "\n" for name in (cpuc.NAMES[3], cpuc.NAMES[0], cpuc.NAMES[2])))
    _patterns(host, PatternBackend, ["-d", pk, "-o", out3, "--top", "0", "-f", str(flist), "--splits"])
    from dandd_amd.host.compat import load_tree
    tree = load_tree(pk)
    sub = [u for f in tree.progressive_fastas(str(flist)) for u in universe if u[0] == f]
    assert len(sub) == 3
    want3 = tables(sub, [int(tree.root_k())], top=0, splits=True)
    assert read_csvs(out3) == want3 and want3["splits"] == []                # (three genomes: no side of two on both sides)


def test_exits(host, tmp_path):
    import test_deltadelta as dd
    pk = ex.exact_tree(str(tmp_path), host)
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            _patterns(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("patterns: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*patterns*")) and not glob.glob(os.path.join(str(e), "*splits*"))
    fails(PatternBackend, ["-d", pk, "-k", "0"], "-k 0", "1..64")
    fails(PatternBackend, ["-d", pk, "-k", "65"], "-k 65", "1..64")
    fails(PatternBackend, ["-d", pk, "--top", "-1"], "--top")
    # more patterns than --max-patterns, where the whole table is asked for: the count is in the message
    universe = golden_universe(str(tmp_path / "data"))
    npat = len(tables(universe, [9], top=0)["patterns"])
    assert npat > 4
    fails(PatternBackend, ["-d", pk, "-k", "9", "--top", "0", "--max-patterns", "4"], f"{npat} patterns", "k=9", "--max-patterns 4")
    fails(PatternBackend, ["-d", pk, "-k", "9", "--splits", "--max-patterns", str(npat - 1)], f"{npat} patterns")
    # ... but the largest rows of a table that large can be had, with the summary's sums over the whole table left empty
    out = str(tmp_path / "big")
    _patterns(host, PatternBackend, ["-d", pk, "-k", "9", "--top", "2", "--max-patterns", "4", "-o", out])
    got = read_csvs(out)
    want = tables(universe, [9], top=2)
    assert got["patterns"] == want["patterns"]
    assert got["patterns_summary"][0][:5] == want["patterns_summary"][0][:5] and got["patterns_summary"][0][5:7] == ["", ""]
    # a backend without the entry, and one without a table for these leaves
    fails(cpus.ScreenBackend, ["-d", pk], "pattern_counts", "exact membership masks")
    fails(NoPatternMasks, ["-d", pk], "no membership masks")
    # a tree of sketches: the message `core` gives
    sk = tmp_path / "sk"
    sk.mkdir()
    _, pks = dd._tree(str(sk), host)
    fails(PatternBackend, ["-d", pks], "tree --exact", "inclusion-exclusion")
    # a tree built over a k window: a k outside it
    from dandd_amd.host import cli
    win = str(tmp_path / "win")
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", str(tmp_path / "data"), "-o", win, "-s", "gold", "-k", "10", "--exact", "--ksweep", "--mink", "8", "--maxk", "11"])
    pkw = glob.glob(os.path.join(win, "*dtree.pickle"))[0]
    fails(PatternBackend, ["-d", pkw, "-k", "12"], "-k 12", "8..11")
    fails(PatternBackend, ["-d", pkw, "-k", "9", "-k", "7"], "-k 7", "8..11")
    # 65 tiny genomes
    many = str(tmp_path / "many")
    os.makedirs(many)
    rng = np.random.default_rng(65)
    for i in range(65):
        with open(os.path.join(many, f"t{i:02d}.fasta"), "w") as f:
            f.write(f">t{i}\n" + "".join(rng.choice(list("ACGT"), size=60)) + "\n")
    out = str(tmp_path / "mt")
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", many, "-o", out, "-s", "many", "-k", "10", "--exact"])
    pk65 = glob.glob(os.path.join(out, "*dtree.pickle"))[0]
    fails(PatternBackend, ["-d", pk65], "65 genomes", "at most 64", "-f")


def test_the_checker_table_is_the_counter_of_the_fixture():
    """table_of, which stands in for the GPU here, on the 7-input fixture the GPU test uses: an identical pair shares every
    bit, the empty file sets none, and the rows are the Counter of the reference's masks in the order of the ABI"""
    for k, canonical in ((11, True), (33, False)):
        _, masks = cpur.reference(k, canonical)
        m, c, found, distinct = table_of(masks)
        assert distinct == len(masks) == int(c.sum()) and found == len(m) == len(set(m.tolist()))
        assert all(int(x) >> 6 == 0 and (int(x) & 1) == (int(x) >> 4 & 1) for x in m)
        assert list(zip(m.tolist(), c.tolist())) == ordered(collections.Counter(masks.values()))
        assert table_of(masks, 3)[0].tolist() == m[:3].tolist() and table_of(masks, 3)[2] == found


def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_patterns", "dd_exact_patterns_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_patterns") and hasattr(engine.Engine, "exact_patterns_device")
    assert engine.Engine.last_patterns_stats is None
    assert hasattr(HipExactBackend, "pattern_counts") and hasattr(DeltaTree, "pattern_tables")
    assert "patterns" in cli.build_parser()._subparsers._group_actions[0].choices and "patterns" in cli.__doc__
