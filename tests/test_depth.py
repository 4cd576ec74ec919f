"""`dandd screen --depth` on the CPU: the entry points of every layer, engine.depth_stats on hand-made arrays and against a
sort of the expanded depths, and the command on the golden exact tree with a checker backend whose depth_hists comes from
depth_ref (test_reads.ReadsBackend plus depth_hists): both CSVs against tables computed from the files' text alone, and the
command's exits.  The GPU's arrays are compared with the same reference in test_gpu_depth.py."""
import csv
import glob
import itertools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import depth_ref
import pyref
import test_core as cpuc
import test_exact_schedules as ex
import test_reads as cpurd
import test_screen as cpus


class DepthBackend(cpurd.ReadsBackend):
    """test_reads.ReadsBackend with depth_hists from depth_ref."""
    name = "exact+core+regions+screen+paint+reads+depth"
    asked = []

    def depth_hists(self, leaf_paths, k, sample_files, all_masks, none_masks, bins):
        n, per_k = self._masks("depth_hists", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        qs = list(zip(all_masks, none_masks))
        type(self).asked.append((qs, int(bins)))
        got = [depth_ref.answer(cpus.text_of(f), int(k), self.canonical, per_k[0], n, qs, int(bins)) for f in sample_files]
        return (np.array([h for h, _ in got], dtype=np.uint64).reshape(len(sample_files), n + len(qs), int(bins)),
                np.array([t for _, t in got], dtype=np.uint64).reshape(len(sample_files), n + len(qs)))


class NoDepthMasks(DepthBackend):
    name = "exact+nodepth"

    def depth_hists(self, leaf_paths, k, sample_files, all_masks, none_masks, bins):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_depth(outdir, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".depth*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == depth_ref.COLS[name], name
        got[name] = body[1:]
    return got


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_depth", "dd_exact_depth_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_depth.hip" in build.SOURCES
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_depth") and hasattr(engine.Engine, "exact_depth_device") and hasattr(engine, "depth_stats")
    assert engine.Engine.last_depth_found is None
    assert hasattr(HipExactBackend, "depth_hists") and hasattr(DeltaTree, "depth_tables")
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "--depth", "--depth-bins", "16", "--depth-hist", "s.fa"])
    assert args.depth is True and args.depth_bins == 16 and args.depth_hist is True
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "s.fa"])
    assert args.depth is False and args.depth_bins is None and args.depth_hist is False
    assert "--depth" in cli.__doc__ and "--depth-bins" in cli.__doc__ and "--depth-hist" in cli.__doc__
    assert cli.DEPTH_COLUMNS == depth_ref.COLS["depth"]


# ---- 2. histograms -> statistics ---------------------------------------------------------------------------------------------
def _row(st, i):
    """row i of depth_stats' arrays in depth_ref.stats' order, NaN as None"""
    def cell(v):
        v = v.item()
        return None if isinstance(v, float) and math.isnan(v) else v
    return tuple(cell(st[name][i]) for name in ("kmers", "covered", "breadth", "mean", "mean_covered", "median", "median_covered", "clipped"))


def test_depth_stats_on_hand_made_arrays():
    from dandd_amd.engine import depth_stats
    hist = np.array([[0, 0, 0, 0],      # an empty row
                     [5, 0, 0, 0],      # nothing of the row is in the sample
                     [1, 1, 1, 3],      # both medians in the clipped bin
                     [2, 1, 1, 0],      # even: the lower of the two middle ones
                     [2, 2, 1, 0],      # odd
                     [4, 0, 0, 1],      # the median over all is 0, the covered one is clipped
                     [0, 0, 7, 0]], dtype=np.uint64)
    total = np.array([0, 0, 20, 3, 4, 900, 14], dtype=np.uint64)
    st = depth_stats(hist, total)
    assert st["kmers"].dtype == np.int64 and st["covered"].dtype == np.int64 and st["clipped"].dtype == np.bool_
    assert all(st[name].dtype == np.float64 for name in ("breadth", "mean", "mean_covered", "median", "median_covered"))
    assert all(v.shape == (7,) for v in st.values())
    assert _row(st, 0) == (0, 0, None, None, None, None, None, False)
    assert _row(st, 1) == (5, 0, 0.0, 0.0, None, 0.0, None, False)
    assert _row(st, 2) == (6, 5, 5 / 6, 20 / 6, 4.0, 2.0, 3.0, True)
    assert _row(st, 3) == (4, 2, 0.5, 0.75, 1.5, 0.0, 1.0, False)
    assert _row(st, 4) == (5, 3, 0.6, 0.8, 4 / 3, 1.0, 1.0, False)
    assert _row(st, 5) == (5, 1, 0.2, 180.0, 900.0, 0.0, 3.0, True)
    assert _row(st, 6) == (7, 7, 1.0, 2.0, 2.0, 2.0, 2.0, False)
    # leading indices of any shape; two bins are the least
    st = depth_stats(hist.reshape(7, 1, 4)[:6].reshape(2, 3, 4), total[:6].reshape(2, 3))
    assert st["median"].shape == (2, 3) and _row({k: v.reshape(-1) for k, v in st.items()}, 5) == (5, 1, 0.2, 180.0, 900.0, 0.0, 3.0, True)
    st = depth_stats([[3, 2]], [9])
    assert _row(st, 0) == (5, 2, 0.4, 1.8, 4.5, 0.0, 1.0, True)
    with pytest.raises(ValueError):
        depth_stats([[3]], [0])
    with pytest.raises(ValueError):
        depth_stats(hist, total[:3])
    # ... and it is the reference's rule: a sort of the expanded depths, for every histogram of four bins with 0..3 in each
    hists = list(itertools.product(range(4), repeat=4))
    totals = [sum(d * v for d, v in enumerate(h)) + 5 * h[3] for h in hists]
    st = depth_stats(hists, totals)
    want = [depth_ref.stats(list(h), t) for h, t in zip(hists, totals)]
    assert [_row(st, i) for i in range(len(hists))] == want
    assert {w[5] for w in want} == {None, 0, 1, 2, 3} and {w[6] for w in want} == {None, 1, 2, 3}


# ---- 3. the command ----------------------------------------------------------------------------------------------------------
def _deep_sample(tmp_path, data):
    """g1 three times over, its first 500 bases nine times more, and a stretch of g2: depths 1, 3 and 12 at the least"""
    g1, g2 = (b"".join(pyref.records(open(os.path.join(data, f"g{g}.fasta"), "rb").read())).decode() for g in (1, 2))
    recs = [g1] * 3 + [g1[:500]] * 9 + [g2[100:900]]
    path = str(tmp_path / "samples" / "deep.fa")
    with open(path, "w") as f:
        f.write("".join(f">d{j}\n{r}\n" for j, r in enumerate(recs)))
    return path


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    s = cpus.make_samples(tmp_path, data)
    deep = _deep_sample(tmp_path, data)
    order = [s["leaf"], s["rel"], deep, s["far"], s["none"]]
    ks = [9, 20]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    cpus._screen(host, DepthBackend, ["-d", pk, "-g", gfile, "-k", "9", "-k", "20", "-o", plain, *order])
    assert not glob.glob(os.path.join(plain, "*depth*"))
    DepthBackend.reset()
    DepthBackend.asked = []
    cpus._screen(host, DepthBackend, ["-d", pk, "-g", gfile, "-k", "20", "-k", "9", "-o", out, "--depth", "--depth-bins", "8", "--depth-hist", *order])
    assert DepthBackend.calls == {"screen_counts": len(ks), "depth_hists": len(ks)}
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    n = len(universe)
    assert DepthBackend.asked == [(depth_ref.query_list(n, groups), 8)] * len(ks)
    # the screen files are what they are without --depth, byte for byte
    for path in glob.glob(os.path.join(plain, "*.screen*.csv")):
        assert open(path, "rb").read() == open(os.path.join(out, os.path.basename(path)), "rb").read(), path
    texts = [(p, cpus.text_of(p)) for p in order]
    want = depth_ref.tables(universe, texts, ks, groups, bins=8)
    got = read_depth(out)
    assert sorted(got) == ["depth", "depth_hist"]
    for name in want:
        assert got[name] == want[name], name
    per = 2 * n + 2 + 3 * len(groups)
    assert len(got["depth"]) == len(order) * len(ks) * per
    col = {c: i for i, c in enumerate(depth_ref.COLS["depth"])}
    at = {(r[0], int(r[1]), os.path.basename(r[2]), r[3]): r for r in got["depth"]}
    for k in ks:
        # a sample that is a leaf: all of it once
        r = at[(s["leaf"], k, "g1.fasta", "all")]
        assert r[col["breadth"]] == "1.0" and r[col["median_depth"]] == "1" and r[col["clipped"]] == "False" and r[col["kmers"]] == r[col["covered"]]
        # the deep sample: g1 at three times or more, its median clipped nowhere, its maximum in the last bin
        r = at[(deep, k, "g1.fasta", "all")]
        assert r[col["breadth"]] == "1.0" and r[col["median_depth"]] == "3" and float(r[col["mean_depth"]]) > 3
        assert [h[4] for h in got["depth_hist"] if h[:4] == [deep, str(k), universe[1][0], "all"]][-1] == ">=7"
        # a sample that shares nothing and an empty one: every k-mer in bin 0, the covered columns empty
        for name in (s["far"], s["none"]):
            r = at[(name, k, "pan", "all")]
            assert r[col["covered"]] == "0" and r[col["breadth"]] == "0.0" and r[col["mean_covered"]] == "" and r[col["median_covered"]] == ""
            assert [h[4:] for h in got["depth_hist"] if h[:4] == [name, str(k), "pan", "all"]] == [["0", r[col["kmers"]]]]
    # the rows of a sample and k, in order
    mine = [r[2:4] for r in got["depth"] if r[0] == deep and r[1] == "9"]
    assert mine == ([[name, cls] for name, _ in universe for cls in ("all", "private")] + [["pan", "all"], ["core", "all"]]
                    + [[label, cls] for label, _ in groups for cls in depth_ref.CLASSES])
    # --depth alone: 64 bins, no histogram file, no group rows without -g
    out2 = str(tmp_path / "o2")
    DepthBackend.asked = []
    cpus._screen(host, DepthBackend, ["-d", pk, "-k", "20", "-o", out2, "--depth", deep, s["rel"]])
    assert DepthBackend.asked == [(depth_ref.query_list(n, None), 64)]
    got2 = read_depth(out2)
    want2 = depth_ref.tables(universe, [(deep, cpus.text_of(deep)), (s["rel"], cpus.text_of(s["rel"]))], [20], None, bins=64)
    assert sorted(got2) == ["depth"] and got2["depth"] == want2["depth"] and len(got2["depth"]) == 2 * (2 * n + 2)


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
        assert not glob.glob(os.path.join(str(e), "*screen*")) and not glob.glob(os.path.join(str(e), "*depth*"))
    fails(DepthBackend, ["-d", pk, "--depth-hist", s["rel"]], "--depth-hist goes with --depth")
    fails(DepthBackend, ["-d", pk, "--depth-bins", "16", s["rel"]], "--depth-bins goes with --depth")
    fails(DepthBackend, ["-d", pk, "--depth", "--depth-bins", "1", s["rel"]], "--depth-bins 1")
    fails(DepthBackend, ["-d", pk, "--depth", "--depth-bins", "257", s["rel"]], "--depth-bins 257")
    fails(cpurd.ReadsBackend, ["-d", pk, "--depth", s["rel"]], "depth_hists", "exact membership masks")
    fails(NoDepthMasks, ["-d", pk, "--depth", s["rel"]], "no membership masks")
