"""`dandd screen --cover` on the CPU: the entry points of every layer, engine.cover_states on hand-made arrays, and the command
on the golden exact tree with a checker backend whose cover_counts comes from cover_ref (test_depth.DepthBackend plus
cover_counts): the three CSVs against tables computed from the files' text alone, and the command's exits.  The GPU's
counters are compared with the same reference in test_gpu_cover.py."""
import csv
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cover_ref
import depth_ref
import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_depth as cpud
import test_exact_schedules as ex
import test_screen as cpus


class CoverBackend(cpud.DepthBackend):
    """test_depth.DepthBackend with cover_counts from cover_ref."""
    name = "exact+core+regions+screen+paint+reads+depth+cover"
    cover_asked = []

    def cover_counts(self, leaf_paths, k, sample_files, window, targets, clip):
        n, per_k = self._masks("cover_counts", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        type(self).cover_asked.append((int(window), [int(t) for t in targets], int(clip)))
        masks = per_k[0]
        fas = [open(json.load(open(row[0]))["fastas"][0], "rb").read() for row in leaf_paths]
        depths = [depth_ref.depths(cpus.text_of(f), int(k), self.canonical, masks) for f in sample_files]
        index, counts = [], []
        for g in targets:
            lens, starts, ntok = cpur.index_of(fas[g])
            index.append((cpur.header_names(fas[g]), np.array(lens, dtype=np.uint64), np.array(starts, dtype=np.uint64), ntok))
            ends = cpur.ends_of(fas[g], int(k), self.canonical)
            nwin = -(-ntok // int(window))
            counts.append(np.array([cover_ref.rows(ends, g, ntok, d, masks, int(window), int(clip)) for d in depths],
                                   dtype=np.uint32).reshape(len(sample_files), nwin, 6))
        return index, counts


class NoCoverMasks(CoverBackend):
    name = "exact+nocover"

    def cover_counts(self, leaf_paths, k, sample_files, window, targets, clip):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_cover(outdir, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".cover*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == cover_ref.COLS[name], name
        got[name] = body[1:]
    return got


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_cover", "dd_exact_cover_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_cover.hip" in build.SOURCES
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_cover") and hasattr(engine.Engine, "exact_cover_device") and hasattr(engine, "cover_states")
    assert engine.Engine.last_cover_found is None
    assert (engine.COVER_EMPTY, engine.COVER_PRESENT, engine.COVER_ABSENT) == (0, 1, 2)
    assert hasattr(HipExactBackend, "cover_counts") and hasattr(DeltaTree, "cover_tables")
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "--cover", "192", "--cover-fastas", "l.txt", "--cover-clip", "7",
                                          "--cover-min", "80", "s.fa"])
    assert args.cover == 192 and args.cover_fastas == "l.txt" and args.cover_clip == 7 and args.cover_min == 80
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "s.fa"])
    assert args.cover is None and args.cover_fastas is None and args.cover_clip is None and args.cover_min is None
    assert all(flag in cli.__doc__ for flag in ("--cover W", "--cover-fastas", "--cover-clip", "--cover-min"))
    assert cli.COVER_COLUMNS == cover_ref.COLS and cli.COVER_STATES == cover_ref.STATES


# ---- 2. rows -> states and runs ----------------------------------------------------------------------------------------------
def test_cover_states_on_hand_made_arrays():
    from dandd_amd.engine import cover_states

    def rows(*pairs):
        return np.array([[v, c, 3 * c, 0, 0, 0] for v, c in pairs], dtype=np.uint32)
    body = rows((64, 64), (64, 32), (64, 31), (0, 0), (64, 0), (64, 1), (200, 1), (200, 2), (64, 63))
    for p in (1, 50, 100):
        states, runs = cover_states(body, p)
        assert states.dtype == np.int64 and states.shape == (9,) and runs.dtype == np.int64 and runs.shape[1] == 3
        w_states, w_runs = cover_ref.states(body.tolist(), p)
        assert states.tolist() == w_states and [tuple(r) for r in runs.tolist()] == w_runs, p
    # 50 %: half is present, one position under half is absent; the window without a valid k-mer is empty whatever it holds
    assert cover_states(body, 50)[0].tolist() == [1, 1, 2, 0, 2, 2, 2, 2, 1]
    # 1 %: one position of 64 is present, one of 200 is not (100 * 1 < 1 * 200), two of 200 are -- the rule is in integers
    assert cover_states(body, 1)[0].tolist() == [1, 1, 1, 0, 2, 1, 2, 1, 1]
    # 100 %: every position or absent
    assert cover_states(body, 100)[0].tolist() == [1, 2, 2, 0, 2, 2, 2, 2, 2]
    # a run does not go on across an empty window: absent | empty | absent are three runs, not one
    states, runs = cover_states(body, 100)
    assert runs.tolist() == [[1, 0, 1], [2, 1, 2], [0, 3, 1], [2, 4, 5]]
    assert cover_states(rows((64, 0), (0, 0), (0, 0), (64, 0)), 50)[1].tolist() == [[2, 0, 1], [0, 1, 2], [2, 3, 1]]
    # one window; none; numbers past 16 bits; a float would round 100 * 21474837 / 2147483647 to 1 %, the integers do not
    assert cover_states(rows((5, 5)), 50)[1].tolist() == [[1, 0, 1]]
    states, runs = cover_states(np.zeros((0, 6), dtype=np.uint32), 50)
    assert states.shape == (0,) and runs.shape == (0, 3)
    assert cover_states(rows((4_000_000_000, 40_000_000), (4_000_000_000, 39_999_999)), 1)[0].tolist() == [1, 2]
    for bad in (0, 101, -1):
        with pytest.raises(ValueError):
            cover_states(body, bad)


# ---- 3. the command ----------------------------------------------------------------------------------------------------------
def _partial_sample(tmp_path, data):
    """g1 with bases 1024..2047 cut out, its first 400 bases five times more, and a stretch of g3: absent windows in g1, a
    depth past the clip, a genome that is mostly absent"""
    g1, g3 = (b"".join(pyref.records(open(os.path.join(data, f"g{g}.fasta"), "rb").read())).decode() for g in (1, 3))
    recs = [g1[:1024], g1[2048:]] + [g1[:400]] * 5 + [g3[300:700]]
    path = str(tmp_path / "samples" / "partial.fa")
    with open(path, "w") as f:
        f.write("".join(f">p{j}\n{r}\n" for j, r in enumerate(recs)))
    return path


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    partial = _partial_sample(tmp_path, data)
    order = [s["leaf"], partial, s["rel"], s["far"], s["none"]]
    ks = [9, 20]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    cpus._screen(host, CoverBackend, ["-d", pk, "-k", "9", "-k", "20", "-o", plain, *order])
    assert not glob.glob(os.path.join(plain, "*cover*"))
    CoverBackend.reset()
    CoverBackend.cover_asked = []
    cpus._screen(host, CoverBackend, ["-d", pk, "-k", "20", "-k", "9", "-o", out, "--cover", "64", "--cover-clip", "3", *order])
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    n = len(universe)
    assert CoverBackend.calls == {"screen_counts": len(ks), "cover_counts": len(ks)}
    assert CoverBackend.cover_asked == [(64, list(range(n)), 3)] * len(ks)
    # the screen files are what they are without --cover, byte for byte
    for path in glob.glob(os.path.join(plain, "*.screen*.csv")):
        assert open(path, "rb").read() == open(os.path.join(out, os.path.basename(path)), "rb").read(), path
    texts = [(p, cpus.text_of(p)) for p in order]
    want = cover_ref.tables(universe, texts, ks, 64, clip=3, min_percent=50)
    got = read_cover(out)
    assert sorted(got) == ["cover", "cover_regions", "cover_summary"]
    for name in want:
        assert got[name] == want[name], name
    ntoks = [cpur.index_of(fa)[2] for _, fa in universe]
    assert len(got["cover"]) == len(order) * len(ks) * sum(-(-t // 64) for t in ntoks)
    assert len(got["cover_summary"]) == len(order) * len(ks) * n
    col = {c: i for i, c in enumerate(cover_ref.COLS["cover"])}
    reg = {c: i for i, c in enumerate(cover_ref.COLS["cover_regions"])}
    smy = {c: i for i, c in enumerate(cover_ref.COLS["cover_summary"])}
    g1 = universe[1][0]
    for k in ks:
        # a sample that is a leaf covers that leaf everywhere, once: breadth 1, depth = covered, no absent window
        r = [r for r in got["cover_summary"] if r[:3] == [s["leaf"], str(k), g1]][0]
        assert r[smy["breadth"]] == "1.0" and r[smy["valid"]] == r[smy["covered"]] and r[smy["absent_windows"]] == "0"
        assert int(r[smy["depth"]]) >= int(r[smy["covered"]]) and r[smy["longest_absent_windows"]] == "0"   # (the golden genomes hold repeats)
        # the partial sample: the cut is ONE absent run of g1 inside windows 16..32, the head is clipped at 3, private positions are covered
        runs = [r for r in got["cover_regions"] if r[:3] == [partial, str(k), g1]]
        absent = [r for r in runs if r[reg["state"]] == "absent"]
        assert len(absent) == 1 and 16 <= int(absent[0][reg["first_window"]]) <= 17 and 14 <= int(absent[0][reg["windows"]]) <= 16
        assert int(absent[0][reg["covered"]]) < int(absent[0][reg["valid"]]) and [r[reg["state"]] for r in runs] == ["present", "absent", "present"]
        assert sum(int(r[reg["windows"]]) for r in runs) == -(-ntoks[1] // 64)
        for a, b in zip(runs, runs[1:]):
            assert int(b[reg["first_window"]]) == int(a[reg["first_window"]]) + int(a[reg["windows"]])
        wins = [r for r in got["cover"] if r[:3] == [partial, str(k), g1]]
        assert wins[1][col["depth"]] == str(3 * int(wins[1][col["covered"]])) and wins[1][col["covered"]] == wins[1][col["valid"]] == "64"
        assert int(wins[20][col["covered"]]) < 32 and wins[20][col["valid"]] == "64" and (k == 9 or wins[20][col["covered"]] == "0")
        assert int(wins[40][col["depth"]]) >= int(wins[40][col["covered"]]) == 64
        r = [r for r in got["cover_summary"] if r[:3] == [partial, str(k), g1]][0]
        assert r[smy["longest_absent_windows"]] == absent[0][reg["windows"]] and 0.9 < float(r[smy["breadth"]]) < 0.97   # (1 kbp of 20 are cut)
        if k == 20:
            assert int(r[smy["private_covered"]]) > 0 and float(r[smy["private_mean_covered_depth"]]) > 1
        # a sample that shares nothing and an empty one: no window present, the ratios over the covered positions are empty cells
        for name in (s["far"], s["none"]):
            r = [r for r in got["cover_summary"] if r[:3] == [name, str(k), g1]][0]
            assert r[smy["covered"]] == "0" and r[smy["breadth"]] == "0.0" and r[smy["mean_covered_depth"]] == "" and r[smy["present_windows"]] == "0"
            assert r[smy["private_mean_covered_depth"]] == ""
    # the valid and private columns do not depend on the sample
    for c in ("valid", "private"):
        per = [[r[col[c]] for r in got["cover"] if r[0] == p] for p in order]
        assert all(x == per[0] for x in per)
    # the rows of a sample and k, in order: genome by genome, window by window
    mine = [(r[2], int(r[3])) for r in got["cover"] if r[0] == partial and r[1] == "9"]
    assert mine == [(name, w) for (name, _), t in zip(universe, ntoks) for w in range(-(-t // 64))]
    # --cover-fastas: two genomes, in the file's order; a wider window; --cover-min 100; the default clip
    lst = tmp_path / "targets.txt"
    lst.write_text(f"g3.fasta\n{universe[1][0]}\n")
    out2 = str(tmp_path / "o2")
    CoverBackend.cover_asked = []
    cpus._screen(host, CoverBackend, ["-d", pk, "-k", "20", "-o", out2, "--cover", "192", "--cover-fastas", str(lst), "--cover-min", "100", partial,
                                      s["leaf"]])
    assert CoverBackend.cover_asked == [(192, [3, 1], 255)]
    got2 = read_cover(out2)
    want2 = cover_ref.tables(universe, [(partial, cpus.text_of(partial)), (s["leaf"], cpus.text_of(s["leaf"]))], [20], 192, targets=[3, 1], clip=255,
                             min_percent=100)
    assert sorted(got2) == ["cover", "cover_regions", "cover_summary"] and all(got2[name] == want2[name] for name in want2)
    assert [r[2] for r in got2["cover_summary"]] == [universe[3][0], universe[1][0]] * 2
    assert any(int(r[col["covered"]]) > 0 and int(r[col["depth"]]) >= 6 * int(r[col["covered"]]) for r in got2["cover"] if r[0] == partial)


def test_exits(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    e = tmp_path / "e"
    twice, stranger, nothing = tmp_path / "twice.txt", tmp_path / "stranger.txt", tmp_path / "nothing.txt"
    twice.write_text("g1.fasta\ng2.fasta\ng1.fasta\n")
    stranger.write_text("g9.fasta\n")
    nothing.write_text("\n")
    few = tmp_path / "few.txt"
    few.write_text(f"{os.path.join(data, 'g0.fasta')}\n{os.path.join(data, 'g1.fasta')}\n")     # (-f takes the leaves' paths)

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            cpus._screen(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("screen: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*screen*")) and not glob.glob(os.path.join(str(e), "*cover*"))
    fails(CoverBackend, ["-d", pk, "--cover", "100", s["rel"]], "--cover 100", "multiple of 64")
    fails(CoverBackend, ["-d", pk, "--cover", "0", s["rel"]], "--cover 0", "multiple of 64")
    fails(CoverBackend, ["-d", pk, "--cover", str((1 << 22) + 64), s["rel"]], "--cover", "multiple of 64")
    fails(CoverBackend, ["-d", pk, "--cover-clip", "7", s["rel"]], "--cover-clip goes with --cover")
    fails(CoverBackend, ["-d", pk, "--cover-min", "7", s["rel"]], "--cover-min goes with --cover")
    fails(CoverBackend, ["-d", pk, "--cover-fastas", str(few), s["rel"]], "--cover-fastas goes with --cover")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-clip", "0", s["rel"]], "--cover-clip 0", "1..1023")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-clip", "1024", s["rel"]], "--cover-clip 1024", "1..1023")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-min", "0", s["rel"]], "--cover-min 0", "1..100")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-min", "101", s["rel"]], "--cover-min 101", "1..100")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-fastas", str(tmp_path / "gone.txt"), s["rel"]], "gone.txt", "not found")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-fastas", str(twice), s["rel"]], "g1.fasta", "stands twice")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-fastas", str(stranger), s["rel"]], "g9.fasta", "is not a leaf of the tree")
    fails(CoverBackend, ["-d", pk, "--cover", "64", "--cover-fastas", str(nothing), s["rel"]], "names no genome")
    fails(CoverBackend, ["-d", pk, "-f", str(few), "--cover", "64", "--cover-fastas", str(twice), s["rel"]], "g2.fasta", "is not in the universe")
    fails(cpud.DepthBackend, ["-d", pk, "--cover", "64", s["rel"]], "cover_counts", "exact membership masks")
    fails(NoCoverMasks, ["-d", pk, "--cover", "64", s["rel"]], "no membership masks")


def test_cover_on_a_tree_of_sketches_exits_the_way_depth_does(host, tmp_path, monkeypatch):
    """screen is an exact command whatever its flags: a tree whose tool is not kmc ends it before anything is read"""
    from dandd_amd.host import cli
    pk = ex.exact_tree(str(tmp_path), host)
    real = cli._load_tree

    def sketches(path):
        tree = real(path)
        tree.experiment["tool"] = "dashing"
        return tree
    monkeypatch.setattr(cli, "_load_tree", sketches)
    codes = []
    for flag in (["--depth"], ["--cover", "64"]):
        with pytest.raises(SystemExit) as err:
            cpus._screen(host, CoverBackend, ["-d", pk, *flag, "-o", str(tmp_path / "e"), "s.fa"])
        codes.append(err.value.code)
    assert codes[0] == codes[1] and "tree of sketches" in codes[0]
