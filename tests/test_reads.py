"""`dandd screen --reads` on the CPU: the entry points of every layer, engine.read_classes on hand-made arrays, and the
command on the golden exact tree with a checker backend whose read_calls comes from reads_ref (test_paint.PaintBackend plus
read_calls): both CSVs against tables computed from the files' text alone, and the command's exits.  The GPU's arrays are
compared with the same reference in test_gpu_reads.py."""
import csv
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import reads_ref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as ex
import test_paint as cpup
import test_screen as cpus


class ReadsBackend(cpup.PaintBackend):
    """test_paint.PaintBackend with read_calls from reads_ref."""
    name = "exact+core+regions+screen+paint+reads"
    wanted = []

    def read_calls(self, leaf_paths, k, sample_files, min_hits, want_calls):
        import json
        n, per_k = self._masks("read_calls", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        type(self).wanted.append(bool(want_calls))
        index, per, tally = [], [], []
        for f in sample_files:
            text = cpus.text_of(f)
            lens, starts, ntok = cpur.index_of(text)
            index.append((cpur.header_names(text), np.array(lens, dtype=np.uint64), np.array(starts, dtype=np.uint64), ntok))
            _, calls, sets, _, row = reads_ref.answer(text, int(k), self.canonical, per_k[0], n, starts, int(min_hits))
            per.append((np.array(calls, dtype=np.uint32).reshape(-1, 6), np.array(sets, dtype=np.uint64).reshape(-1, 2)) if want_calls else None)
            tally.append(row)
        return index, per, np.array(tally, dtype=np.uint64).reshape(len(sample_files), n + 3)


class NoReadsMasks(ReadsBackend):
    name = "exact+noreads"

    def read_calls(self, leaf_paths, k, sample_files, min_hits, want_calls):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_reads(outdir, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".reads*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == reads_ref.COLS[name], name
        got[name] = body[1:]
    return got


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_reads", "dd_exact_reads_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_reads.hip" in build.SOURCES
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_reads") and hasattr(engine.Engine, "exact_reads_device") and hasattr(engine, "read_classes")
    assert engine.Engine.last_reads_found is None and engine.NO_GENOME == reads_ref.NONE
    assert hasattr(HipExactBackend, "read_calls") and hasattr(DeltaTree, "reads_tables")
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "--reads", "--reads-calls", "--reads-min-hits", "7", "s.fa"])
    assert args.reads is True and args.reads_calls is True and args.reads_min_hits == 7
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "s.fa"])
    assert args.reads is False and args.reads_calls is False and args.reads_min_hits == 1
    assert "--reads" in cli.__doc__ and "--reads-calls" in cli.__doc__ and "--reads-min-hits" in cli.__doc__


# ---- 2. call arrays -> classes and tally -----------------------------------------------------------------------------------
def test_read_classes_on_hand_made_arrays():
    from dandd_amd.engine import NO_GENOME, read_classes
    X = NO_GENOME
    # valid, hit, best, best_count, second, second_count | ties, full      (n = 3)
    rows = [([0, 0, X, 0, X, 0], [0, 0]),             # no valid k-mer
            ([9, 0, X, 0, X, 0], [0, 0]),             # valid k-mers, none of the universe: unclassified at every min_hits
            ([9, 5, 2, 5, X, 0], [4, 4]),             # unique to genome 2
            ([9, 5, 0, 4, 1, 4], [3, 0]),             # genomes 0 and 1 tie: ambiguous
            ([9, 5, 1, 3, 0, 2], [2, 0]),             # unique to genome 1 with 3 positions
            ([9, 8, 0, 8, 1, 8], [7, 7])]             # all three tie
    calls = np.array([c for c, _ in rows], dtype=np.uint32)
    sets = np.array([s for _, s in rows], dtype=np.uint64)
    classes, tally = read_classes(calls, sets, 1, 3)
    assert classes.dtype == np.int64 and tally.dtype == np.uint64 and tally.shape == (6,)
    assert classes.tolist() == [5, 4, 2, 3, 1, 3] and tally.tolist() == [0, 1, 1, 2, 1, 1]
    classes, tally = read_classes(calls, sets, 4, 3)
    assert classes.tolist() == [5, 4, 2, 3, 4, 3] and tally.tolist() == [0, 0, 1, 2, 2, 1]
    classes, tally = read_classes(calls, sets, 9, 3)
    assert classes.tolist() == [5, 4, 4, 4, 4, 4] and tally.tolist() == [0, 0, 0, 0, 5, 1]
    # bit 63 alone is one genome; without n the tally has the bins of 64 genomes
    classes, tally = read_classes([[1, 1, 63, 1, X, 0]], [[1 << 63, 1 << 63]], 1)
    assert classes.tolist() == [63] and tally.shape == (67,) and tally[63] == 1 and tally.sum() == 1
    classes, tally = read_classes(np.zeros((0, 6), dtype=np.uint32), np.zeros((0, 2), dtype=np.uint64), 1, 3)
    assert classes.shape == (0,) and tally.tolist() == [0] * 6
    with pytest.raises(ValueError):
        read_classes(calls, sets, 0, 3)
    # ... and it is the reference's rule: every row of reads_ref.vote over all small rows of two genomes
    want, calls, sets = [], [], []
    for valid in range(4):
        for a in range(valid + 1):
            for b in range(valid + 1):
                for hit in range(max(a, b), min(valid, a + b) + 1):
                    if hit == 0 and (a or b) or hit and not (a or b):
                        continue
                    c, s, cls = reads_ref.vote([valid, hit, a, b], 2, 2)
                    calls.append(c), sets.append(s), want.append(cls)
    classes, tally = read_classes(calls, sets, 2, 2)
    assert classes.tolist() == want and set(want) == {0, 1, 2, 3, 4} and tally.tolist() == [want.count(c) for c in range(5)]


# ---- 3. the command ----------------------------------------------------------------------------------------------------------
def _reads_sample(tmp_path, data):
    """records of 60 bases cut from g1, g2 and g3 in turn, an empty record, one of 5 bases and one of unrelated text"""
    import pyref
    rng = np.random.default_rng(20261020)
    texts = [b"".join(pyref.records(open(os.path.join(data, f"g{g}.fasta"), "rb").read())).decode() for g in (1, 2, 3)]
    recs = []
    for j in range(18):
        t = texts[j % 3]
        p = int(rng.integers(0, len(t) - 60))
        recs.append(t[p:p + 60])
    recs[7:7] = ["", "ACGTA", "".join(rng.choice(list("ACGT"), size=60))]
    path = str(tmp_path / "samples" / "reads.fa")
    with open(path, "w") as f:
        f.write("".join(f">r{j} x\n{r}\n" for j, r in enumerate(recs)))
    return path


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    reads = _reads_sample(tmp_path, data)
    order = [s["leaf"], s["rel"], reads, s["far"], s["none"]]
    ks = [9, 20]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    cpus._screen(host, ReadsBackend, ["-d", pk, "-k", "9", "-k", "20", "-o", plain, *order])
    assert not glob.glob(os.path.join(plain, "*reads*"))
    ReadsBackend.reset()
    ReadsBackend.wanted = []
    cpus._screen(host, ReadsBackend, ["-d", pk, "-k", "20", "-k", "9", "-o", out, "--reads", "--reads-calls", *order])
    assert ReadsBackend.calls == {"screen_counts": len(ks), "read_calls": len(ks)} and ReadsBackend.wanted == [True] * len(ks)
    # the screen files are what they are without --reads, byte for byte
    for path in glob.glob(os.path.join(plain, "*.screen*.csv")):
        assert open(path, "rb").read() == open(os.path.join(out, os.path.basename(path)), "rb").read(), path
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    texts = [(p, cpus.text_of(p)) for p in order]
    want = reads_ref.tables(universe, texts, ks)
    got = read_reads(out)
    assert sorted(got) == ["reads", "reads_summary"]
    for name in want:
        assert got[name] == want[name], name
    n, nrec = len(universe), [len(cpur.index_of(t)[0]) for _, t in texts]
    assert nrec == [2, 2, 21, 1, 0]
    assert len(got["reads_summary"]) == len(ks) * len(order) * (n + 3) and len(got["reads"]) == len(ks) * sum(nrec)
    col = {c: i for i, c in enumerate(reads_ref.COLS["reads"])}
    mine = [r for r in got["reads"] if r[0] == reads and r[1] == "20"]
    # the fixture does what it is for: unique calls to three genomes, an empty record and a short one without a k-mer, text
    # of no genome unclassified; the leaf is unique to itself, and the sample without a record has empty fractions
    assert {os.path.basename(r[col["best_fasta"]]) for r in mine if r[col["class"]] == "unique"} >= {"g1.fasta", "g2.fasta", "g3.fasta"}
    assert [r[col["class"]] for r in mine[7:10]] == ["no_kmer", "no_kmer", "unclassified"] and mine[7][col["length"]] == "0"
    assert mine[9][col["best_fasta"]] == "" and mine[9][col["ties"]] == "0"
    leaf = [r for r in got["reads"] if r[0] == s["leaf"]]
    assert all(r[col["class"]] == "unique" and os.path.basename(r[col["best_fasta"]]) == "g1.fasta" and r[col["valid"]] == r[col["best_shared"]]
               for r in leaf)
    none = [r for r in got["reads_summary"] if r[0] == s["none"]]
    assert len(none) == len(ks) * (n + 3) and all(r[3] == "0" and r[4] == "" for r in none)
    for sample, t in texts:
        for k in ks:
            rows = [r for r in got["reads_summary"] if r[0] == sample and r[1] == str(k)]
            assert [r[2] for r in rows] == [name for name, _ in universe] + ["ambiguous", "unclassified", "no_kmer"]
            assert sum(int(r[3]) for r in rows) == len(cpur.index_of(t)[0])
    # --reads alone: the summary only, from the tally-only call; a threshold
    out2 = str(tmp_path / "o2")
    ReadsBackend.wanted = []
    cpus._screen(host, ReadsBackend, ["-d", pk, "-k", "20", "-o", out2, "--reads", "--reads-min-hits", "30", reads, s["rel"]])
    assert ReadsBackend.wanted == [False]
    got2 = read_reads(out2)
    want2 = reads_ref.tables(universe, [(reads, cpus.text_of(reads)), (s["rel"], cpus.text_of(s["rel"]))], [20], min_hits=30)
    assert sorted(got2) == ["reads_summary"] and got2["reads_summary"] == want2["reads_summary"]
    assert got2["reads_summary"] != [r for r in got["reads_summary"] if r[0] in (reads, s["rel"]) and r[1] == "20"]


def test_exits(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            cpus._screen(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("screen: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*screen*")) and not glob.glob(os.path.join(str(e), "*reads*"))
    fails(ReadsBackend, ["-d", pk, "--reads-calls", s["rel"]], "--reads-calls goes with --reads")
    fails(ReadsBackend, ["-d", pk, "--reads", "--reads-min-hits", "0", s["rel"]], "--reads-min-hits 0")
    fails(ReadsBackend, ["-d", pk, "--reads", "--reads-min-hits", "-3", s["rel"]], "--reads-min-hits -3")
    fails(cpup.PaintBackend, ["-d", pk, "--reads", s["rel"]], "read_calls", "exact membership masks")
    fails(NoReadsMasks, ["-d", pk, "--reads", s["rel"]], "no membership masks")
