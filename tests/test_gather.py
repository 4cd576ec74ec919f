"""`dandd screen --gather` on the CPU: the entry points of every layer, gather_ref's walk on hand-made records (a tie, a
duplicate genome, both stop rules, the sum identities), and the command on the golden exact tree with a checker backend
whose gather_picks comes from gather_ref (test_depth.DepthBackend plus gather_picks): both CSVs against tables computed from
the files' text alone, and the command's exits.  The GPU's arrays are compared with the same reference in test_gpu_gather.py."""
import csv
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gather_ref
import pyref
import test_core as cpuc
import test_depth as cpud
import test_exact_schedules as ex
import test_screen as cpus


class GatherBackend(cpud.DepthBackend):
    """test_depth.DepthBackend with gather_picks from gather_ref."""
    name = "exact+core+regions+screen+paint+reads+depth+gather"
    walked = []

    def gather_picks(self, leaf_paths, k, sample_files, min_hits, steps):
        n, per_k = self._masks("gather_picks", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        type(self).walked.append((int(min_hits), int(steps)))
        got = [gather_ref.answer(cpus.text_of(f), int(k), self.canonical, per_k[0], n, int(min_hits), int(steps)) for f in sample_files]
        ns = len(sample_files)
        return (np.array([g[0] for g in got], dtype=np.int32).reshape(ns, int(steps)),
                *(np.array([g[j] for g in got], dtype=np.uint64).reshape(ns, cols) for j, cols in ((1, int(steps)), (2, int(steps)), (3, n), (4, 2))))


class NoGatherMasks(GatherBackend):
    name = "exact+nogather"

    def gather_picks(self, leaf_paths, k, sample_files, min_hits, steps):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_gather(outdir, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".gather*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == gather_ref.COLS[name], name
        got[name] = body[1:]
    return got


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_gather", "dd_exact_gather_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_gather.hip" in build.SOURCES
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_gather") and hasattr(engine.Engine, "exact_gather_device")
    assert engine.Engine.last_gather_found is None
    assert hasattr(HipExactBackend, "gather_picks") and hasattr(DeltaTree, "gather_tables")
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "--gather", "--gather-min", "16", "--gather-steps", "3", "s.fa"])
    assert args.gather is True and args.gather_min == 16 and args.gather_steps == 3
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "s.fa"])
    assert args.gather is False and args.gather_min is None and args.gather_steps is None
    assert "--gather" in cli.__doc__ and "--gather-min" in cli.__doc__ and "--gather-steps" in cli.__doc__
    assert cli.GATHER_COLUMNS == gather_ref.COLS


# ---- 2. the walk on hand-made records ----------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_lower_index():
    # inputs 1 and 2 hold three private records each, input 0 two: U_0 = [2, 3, 3]
    held = [(0b010, 1)] * 3 + [(0b100, 5)] * 3 + [(0b001, 2)] * 2
    pick, unique, depth, shared, total = gather_ref.walk(held, 3)
    assert shared == [2, 3, 3] and pick == [1, 2, 0] and unique == [3, 3, 2] and depth == [3, 15, 4] and total == [8, 22]
    # ... and a tie at a later step: behind input 3, inputs 0 and 1 both add two
    held = [(0b1000, 1)] * 5 + [(0b1001, 1), (0b0001, 1), (0b0001, 2), (0b0010, 3), (0b0010, 4)]
    pick, unique, depth, _, _ = gather_ref.walk(held, 4)
    assert pick == [3, 0, 1, -1] and unique == [6, 2, 2, 0] and depth == [6, 3, 7, 0]


def test_a_duplicate_genome_is_never_picked():
    # inputs 2 and 5 are the same genome: every record of one is a record of the other
    dup = 1 << 2 | 1 << 5
    held = [(dup, 2)] * 6 + [(dup | 1, 1)] * 2 + [(1, 1)] * 3 + [(1 << 3, 7)]
    pick, unique, depth, shared, total = gather_ref.walk(held, 6)
    assert shared == [5, 0, 8, 1, 0, 8]
    assert pick == [2, 0, 3, -1, -1, -1] and unique == [8, 3, 1, 0, 0, 0] and depth == [14, 3, 7, 0, 0, 0]
    assert 5 not in pick and sum(unique) == total[0] == 12 and sum(depth) == total[1] == 24


def test_the_stop_rules():
    held = [(0b001, 1)] * 10 + [(0b011, 2)] * 4 + [(0b010, 1)] * 3 + [(0b100, 9)] * 2
    full = gather_ref.walk(held, 3)
    assert full[0] == [0, 1, 2] and full[1] == [14, 3, 2] and full[2] == [18, 3, 18]
    # min_hits between the second and the third pick's unique stops the walk behind the second; at the first's, behind none
    assert gather_ref.walk(held, 3, min_hits=3)[:3] == ([0, 1, -1], [14, 3, 0], [18, 3, 0])
    assert gather_ref.walk(held, 3, min_hits=4)[:3] == ([0, -1, -1], [14, 0, 0], [18, 0, 0])
    assert gather_ref.walk(held, 3, min_hits=15)[:3] == ([-1, -1, -1], [0, 0, 0], [0, 0, 0])
    # steps cuts it: the arrays are `steps` long, the by-products do not change
    for steps in (1, 2):
        got = gather_ref.walk(held, 3, steps=steps)
        assert got[:3] == tuple(a[:steps] for a in full[:3]) and got[3:] == full[3:]
    assert gather_ref.walk([], 3) == ([-1] * 3, [0] * 3, [0] * 3, [0] * 3, [0, 0])


def test_the_sum_identities_on_random_records():
    rng = np.random.default_rng(5)
    for n in (1, 5, 64):
        masks = [int(rng.integers(1, 1 << 62)) & ((1 << n) - 1) or 1 for _ in range(300)]
        held = [(m | (1 << 63 if n == 64 and j % 7 == 0 else 0), int(rng.integers(1, 50))) for j, m in enumerate(masks)]
        pick, unique, depth, shared, total = gather_ref.walk(held, n)
        assert sum(unique) == total[0] == 300 and sum(depth) == total[1] == sum(d for _, d in held)
        assert all(a >= b for a, b in zip(unique, unique[1:]))
        live = [p for p in pick if p >= 0]
        assert len(set(live)) == len(live) and pick[len(live):] == [-1] * (n - len(live))
        assert shared[pick[0]] == unique[0] == max(shared)


# ---- 3. the command ----------------------------------------------------------------------------------------------------------
def _mixture(tmp_path, data):
    """g1 whole, g3 twice over and a stretch of g2: three picks, g3 at depth 2"""
    g = {j: b"".join(pyref.records(open(os.path.join(data, f"g{j}.fasta"), "rb").read())).decode() for j in (1, 2, 3)}
    recs = [g[1], g[3], g[3], g[2][200:1100]]
    path = str(tmp_path / "samples" / "mix.fa")
    with open(path, "w") as f:
        f.write("".join(f">m{j}\n{r}\n" for j, r in enumerate(recs)))
    return path


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    mix = _mixture(tmp_path, data)
    order = [s["leaf"], mix, s["rel"], s["far"], s["none"]]
    ks = [9, 20]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    cpus._screen(host, GatherBackend, ["-d", pk, "-k", "9", "-k", "20", "-o", plain, *order])
    assert not glob.glob(os.path.join(plain, "*gather*"))
    GatherBackend.reset()
    GatherBackend.walked = []
    cpus._screen(host, GatherBackend, ["-d", pk, "-k", "20", "-k", "9", "-o", out, "--gather", *order])
    assert GatherBackend.calls == {"screen_counts": len(ks), "gather_picks": len(ks)}
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    n = len(universe)
    assert GatherBackend.walked == [(1, n)] * len(ks)
    # the screen files are what they are without --gather, byte for byte
    for path in glob.glob(os.path.join(plain, "*.screen*.csv")):
        assert open(path, "rb").read() == open(os.path.join(out, os.path.basename(path)), "rb").read(), path
    texts = [(p, cpus.text_of(p)) for p in order]
    want = gather_ref.tables(universe, texts, ks)
    got = read_gather(out)
    assert sorted(got) == ["gather", "gather_summary"]
    for name in want:
        assert got[name] == want[name], name
    col = {c: i for i, c in enumerate(gather_ref.COLS["gather"])}
    sm = {c: i for i, c in enumerate(gather_ref.COLS["gather_summary"])}
    assert len(got["gather_summary"]) == len(order) * len(ks)
    for k in ks:
        rows = [r for r in got["gather"] if r[0] == mix and r[1] == str(k)]
        # the mixture: its three genomes in front, all of the pan-genome's share explained, g3 held twice
        assert [r[col["rank"]] for r in rows] == [str(j + 1) for j in range(len(rows))] and len(rows) >= 3
        assert {os.path.basename(r[col["fasta"]]) for r in rows[:3]} == {"g1.fasta", "g2.fasta", "g3.fasta"}
        assert rows[-1][col["remaining"]] == "0"
        if k == 20:
            g3 = [r for r in rows if os.path.basename(r[col["fasta"]]) == "g3.fasta"][0]
            assert 2.0 <= float(g3[col["mean_depth"]]) < 2.1             # (twice over, and the few k-mers g3 repeats in itself)
        # a sample that is a leaf: one pick explains it whole
        leaf = [r for r in got["gather"] if r[0] == s["leaf"] and r[1] == str(k)]
        assert os.path.basename(leaf[0][col["fasta"]]) == "g1.fasta" and leaf[0][col["f_sample_unique"]] == "1.0" and leaf[0][col["remaining"]] == "0"
        # a sample that shares nothing and an empty one: no pick, a summary row
        for name in (s["far"], s["none"]):
            assert not [r for r in got["gather"] if r[0] == name and r[1] == str(k)]
            row = [r for r in got["gather_summary"] if r[0] == name and r[1] == str(k)][0]
            assert row[sm["genomes"]] == "0" and row[sm["explained"]] == "0" and row[sm["top_fasta"]] == ""
    # --gather-min and --gather-steps reach the backend and the tables
    out2 = str(tmp_path / "o2")
    GatherBackend.walked = []
    cpus._screen(host, GatherBackend, ["-d", pk, "-k", "20", "-o", out2, "--gather", "--gather-min", "40", "--gather-steps", "2", mix, s["rel"]])
    assert GatherBackend.walked == [(40, 2)]
    got2 = read_gather(out2)
    want2 = gather_ref.tables(universe, [(mix, cpus.text_of(mix)), (s["rel"], cpus.text_of(s["rel"]))], [20], min_hits=40, steps=2)
    assert got2 == want2 and len([r for r in got2["gather"] if r[0] == mix]) == 2


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
        assert not glob.glob(os.path.join(str(e), "*screen*")) and not glob.glob(os.path.join(str(e), "*gather*"))
    fails(GatherBackend, ["-d", pk, "--gather-min", "2", s["rel"]], "--gather-min goes with --gather")
    fails(GatherBackend, ["-d", pk, "--gather-steps", "2", s["rel"]], "--gather-steps goes with --gather")
    fails(GatherBackend, ["-d", pk, "--gather", "--gather-min", "0", s["rel"]], "--gather-min 0")
    fails(GatherBackend, ["-d", pk, "--gather", "--gather-steps", "0", s["rel"]], "--gather-steps 0")
    fails(GatherBackend, ["-d", pk, "--gather", "--gather-steps", "6", s["rel"]], "--gather-steps 6", "5 genomes")
    fails(cpud.DepthBackend, ["-d", pk, "--gather", s["rel"]], "gather_picks", "exact membership masks")
    fails(NoGatherMasks, ["-d", pk, "--gather", s["rel"]], "no membership masks")
