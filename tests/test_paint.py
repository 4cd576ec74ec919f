"""`dandd screen --paint` on the CPU: the entry points of every layer, engine.paint_windows on hand-made record indexes, and
the command on the golden exact tree with a checker backend whose paint_counts comes from paint_ref (test_screen.ScreenBackend
plus paint_counts): the three CSVs against tables computed from the files' text alone, the tie rule of the best genome, the
merging of windows into segments, and the command's exits.  The GPU's counters are compared with the same reference in
test_gpu_paint.py."""
import csv
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import paint_ref
import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as ex
import test_screen as cpus


class PaintBackend(cpus.ScreenBackend):
    """test_screen.ScreenBackend with paint_counts from paint_ref."""
    name = "exact+core+regions+screen+paint"

    def paint_counts(self, leaf_paths, k, sample_files, window):
        import json
        n, per_k = self._masks("paint_counts", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        index, counts = [], []
        for f in sample_files:
            text = cpus.text_of(f)
            lens, starts, ntok = cpur.index_of(text)
            index.append((cpur.header_names(text), np.array(lens, dtype=np.uint64), np.array(starts, dtype=np.uint64), ntok))
            counts.append(np.array(paint_ref.rows(text, int(k), self.canonical, per_k[0], n, int(window)), dtype=np.uint32).reshape(-1, n + 2))
        return index, counts


class NoPaintMasks(PaintBackend):
    name = "exact+nopaint"

    def paint_counts(self, leaf_paths, k, sample_files, window):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_paint(outdir, universe_names, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".paint*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == (paint_ref.COLS[name] if name in paint_ref.COLS else ["sample", "k", "window", *universe_names]), name
        got[name] = body[1:]
    return got


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_paint", "dd_exact_paint_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert "dd_exact_paint.hip" in build.SOURCES
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_paint") and hasattr(engine.Engine, "exact_paint_device") and hasattr(engine, "paint_windows")
    assert engine.Engine.last_paint_found is None
    assert hasattr(HipExactBackend, "paint_counts") and hasattr(DeltaTree, "paint_tables")
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "--paint", "192", "--paint-matrix", "s.fa"])
    assert args.paint == 192 and args.paint_matrix is True
    args = cli.build_parser().parse_args(["screen", "-d", "t.pickle", "s.fa"])
    assert args.paint is None and args.paint_matrix is False
    assert "--paint" in cli.__doc__


# ---- 2. windows -> places in the records -------------------------------------------------------------------------------------
def test_paint_windows_on_hand_made_indexes():
    from dandd_amd.engine import paint_windows
    # three records of 100, 0 and 200 bases: BREAK 0, bases 1..100, BREAK 101 (the empty record's), BREAK 102, bases 103..302
    tok_start, seq_len, ntok = [1, 102, 103], [100, 0, 200], 303

    def rows(window):
        got = paint_windows(-(-ntok // window), window, tok_start, seq_len)
        assert all(a.dtype == np.int64 and a.shape == (-(-ntok // window),) for a in got)
        return [tuple(int(v) for v in row) for row in zip(*got)]
    # W = 64: window 0 holds the first BREAK and bases 0..62; window 1 straddles the records (and the empty one between them,
    # which holds no base and is not counted); windows 2, 3 lie inside record 2; window 4 is the last, partial one
    assert rows(64) == [(0, 0, 63, 1), (0, 63, 100, 2), (2, 25, 89, 1), (2, 89, 153, 1), (2, 153, 200, 1)]
    assert rows(128) == [(0, 0, 100, 2), (2, 25, 153, 1), (2, 153, 200, 1)]
    assert rows(1 << 22) == [(0, 0, 100, 2)]
    # a window of nothing but the BREAKs of empty records; an index without a record; no window
    got = paint_windows(2, 64, [1, 2, 3, 66], [0, 0, 0, 0])
    assert [a.tolist() for a in got] == [[-1, -1], [0, 0], [0, 0], [0, 0]]
    got = paint_windows(1, 64, [1, 2, 3], [0, 0, 5])
    assert [a.tolist() for a in got] == [[2], [0], [5], [1]]
    assert [a.tolist() for a in paint_windows(0, 64, [], [])] == [[], [], [], []]
    # ... and the same places token by token, on the fixture with three records, one of them empty
    g3 = cpur.genomes()[3]
    lens, starts, n = cpur.index_of(g3)
    names = cpur.header_names(g3)
    for window in (64, 192, 4096):
        got = paint_windows(-(-n // window), window, starts, lens)
        mine = [(names[r] if r >= 0 else None, int(s), int(e), int(c)) for r, s, e, c in zip(*got)]
        assert mine == paint_ref.places(g3, window), window


# ---- 3. the command ----------------------------------------------------------------------------------------------------------
def _mosaic(tmp_path, data):
    """half g1, half text that is in no genome"""
    rng = np.random.default_rng(20261020)
    g1 = b"".join(pyref.records(open(os.path.join(data, "g1.fasta"), "rb").read())).decode()
    novel = "".join(rng.choice(list("ACGT"), size=1024))
    novel = "ACGT"[("ACGT".index(g1[1023].upper()) + 1) % 4] + novel[1:]       # (no k-mer of g1 runs on across the border)
    path = str(tmp_path / "samples" / "mosaic.fa")
    with open(path, "w") as f:
        f.write(">mosaic\n" + g1[:1023] + novel + "\n")      # 1 BREAK + 1023 bases: the border falls on a window's
    return path


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = cpus.make_samples(tmp_path, data)
    mosaic = _mosaic(tmp_path, data)
    order = [s["leaf"], s["rel"], mosaic, s["far"], s["none"]]
    ks = [9, 20]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    cpus._screen(host, PaintBackend, ["-d", pk, "-k", "9", "-k", "20", "-o", plain, *order])
    assert not glob.glob(os.path.join(plain, "*paint*"))
    PaintBackend.reset()
    cpus._screen(host, PaintBackend, ["-d", pk, "-k", "20", "-k", "9", "-o", out, "--paint", "64", "--paint-matrix", *order])
    assert PaintBackend.calls == {"screen_counts": len(ks), "paint_counts": len(ks)}
    # the screen files are what they are without --paint, byte for byte
    for path in glob.glob(os.path.join(plain, "*.screen*.csv")):
        assert open(path, "rb").read() == open(os.path.join(out, os.path.basename(path)), "rb").read(), path
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    want = paint_ref.tables(universe, [(p, cpus.text_of(p)) for p in order], ks, 64)
    got = read_paint(out, [name for name, _ in universe])
    assert sorted(got) == ["paint", "paint_matrix", "paint_segments"]
    for name in want:
        assert got[name] == want[name], name
    ntoks = [cpur.index_of(cpus.text_of(p))[2] for p in order]
    assert len(got["paint"]) == len(got["paint_matrix"]) == len(ks) * sum(-(-t // 64) for t in ntoks) and ntoks[4] == 0
    col = {c: i for i, c in enumerate(paint_ref.COLS["paint"])}
    # a tie of the two best genomes stays with the earlier one of the universe
    order_of = {name: i for i, (name, _) in enumerate(universe)}
    ties = [r for r in got["paint"] if r[col["best_shared"]] and r[col["best_shared"]] == r[col["second_shared"]]]
    assert ties and all(order_of[r[col["best_fasta"]]] < order_of[r[col["second_fasta"]]] for r in ties)
    # a leaf byte for byte: nothing novel anywhere, every position is its own genome's
    mine = [r for r in got["paint"] if r[0] == s["leaf"]]
    g1 = [r[3 + 1] for r in got["paint_matrix"] if r[0] == s["leaf"]]
    assert all(r[col["novel"]] == "0" for r in mine) and g1 == [r[col["valid"]] for r in mine]
    # two records: a window that straddles them says so
    assert {r[col["records"]] for r in got["paint"] if r[0] == s["rel"]} == {"1", "2"}
    # segments: the runs of the mosaic at k = 20 are consecutive and maximal, each is the sum of its windows, and the novel half
    # (windows 16..31: every k-mer that ends there holds a base of the unrelated text) is ONE run with an empty best_fasta
    seg = {c: i for i, c in enumerate(paint_ref.COLS["paint_segments"])}
    runs = [r for r in got["paint_segments"] if r[0] == mosaic and r[1] == "20"]
    wins = [r for r in got["paint"] if r[0] == mosaic and r[1] == "20"]
    assert len(wins) == 32 and ntoks[2] == 2048
    assert runs[0][seg["first_window"]] == "0" and runs[-1][seg["last_window"]] == "31"
    for a, b in zip(runs, runs[1:]):
        assert int(b[seg["first_window"]]) == int(a[seg["last_window"]]) + 1 and a[seg["best_fasta"]] != b[seg["best_fasta"]]
        assert a[seg["tok_end"]] == b[seg["tok_start"]] == str(64 * int(b[seg["first_window"]]))
    for r in runs:
        mine = wins[int(r[seg["first_window"]]):int(r[seg["last_window"]]) + 1]
        assert {w[col["best_fasta"]] for w in mine} == {r[seg["best_fasta"]]}
        for c in ("valid", "in_pan"):
            assert int(r[seg[c]]) == sum(int(w[col[c]]) for w in mine)
        assert r[seg["best_shared"]] == ("" if not r[seg["best_fasta"]] else str(sum(int(w[col["best_shared"]]) for w in mine)))
    assert [runs[-1][seg[c]] for c in ("first_window", "last_window", "tok_start", "tok_end", "best_fasta", "in_pan", "best_shared")] == \
        ["16", "31", "1024", "2048", "", "0", ""]
    assert all(r[seg["best_fasta"]] for r in runs[:-1]) and any(os.path.basename(r[seg["best_fasta"]]) == "g1.fasta" for r in runs)
    assert sum(int(r[seg["valid"]]) for r in runs) == 2047 - 20 + 1 and len(runs) < 17
    assert len(got["paint_segments"]) < len(got["paint"])
    # without --paint-matrix: two files; a wider window
    out2 = str(tmp_path / "o2")
    cpus._screen(host, PaintBackend, ["-d", pk, "-k", "9", "-o", out2, "--paint", "192", s["rel"], mosaic])
    got = read_paint(out2, [name for name, _ in universe])
    want = paint_ref.tables(universe, [(p, cpus.text_of(p)) for p in (s["rel"], mosaic)], [9], 192)
    assert sorted(got) == ["paint", "paint_segments"] and all(got[name] == want[name] for name in got)


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
        assert not glob.glob(os.path.join(str(e), "*screen*")) and not glob.glob(os.path.join(str(e), "*paint*"))
    fails(PaintBackend, ["-d", pk, "--paint", "100", s["rel"]], "--paint 100", "multiple of 64")
    fails(PaintBackend, ["-d", pk, "--paint", "0", s["rel"]], "--paint 0", "multiple of 64")
    fails(PaintBackend, ["-d", pk, "--paint", str((1 << 22) + 64), s["rel"]], "--paint", "multiple of 64")
    fails(PaintBackend, ["-d", pk, "--paint-matrix", s["rel"]], "--paint-matrix goes with --paint")
    fails(cpus.ScreenBackend, ["-d", pk, "--paint", "64", s["rel"]], "paint_counts", "exact membership masks")
    fails(NoPaintMasks, ["-d", pk, "--paint", "64", s["rel"]], "no membership masks")
