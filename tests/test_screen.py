"""`dandd screen` on the CPU: the entry points of every layer, and the command on the golden exact tree with a checker backend
whose screen_counts comes from Python sets of pyref.kmers (test_core_regions.RegionBackend plus screen_counts, and a card
that answers the samples' own counts): the three CSVs against tables computed here from the files' text alone, and the
command's exits.  The GPU's tables are compared with the same sets in test_gpu_screen.py."""
import csv
import glob
import gzip
import io
import json
import os
import re
import shutil
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import pyref
import test_core as cpuc
import test_core_regions as cpur
import test_exact_schedules as ex

CLASSES = ("core", "private", "signature")
COLS = {
    "screen": ["sample", "k", "fasta", "genome_kmers", "sample_kmers", "shared", "genome_containment", "sample_containment", "jaccard"],
    "screen_summary": ["sample", "k", "sample_kmers", "in_pan", "novel", "in_core", "best_fasta", "best_jaccard", "best_genome_containment"],
    "screen_groups": ["sample", "k", "group", "class", "marker_kmers", "hits", "fraction"],
}


def text_of(path):
    """a sample's text: the file's bytes, inflated when they are gzip"""
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def cell(v):
    return "" if v is None else str(v)


def ratio(a, b):
    return a / b if b else None


def tables(universe, samples, ks, groups, canonical=True):
    """The three files of `screen` as lists of rows of strings, from sets of pyref.kmers over the texts alone.
    universe: [(name as the CSV shows it, FASTA bytes)], samples: [(name, text)], groups: [(label, members)] or None."""
    n = len(universe)
    full = (1 << n) - 1
    rows, summary, marks = [], [], []
    for sname, text in samples:
        for k in ks:
            G = [set(pyref.kmers(fa, k, canonical)) for _, fa in universe]
            Q = set(pyref.kmers(text, k, canonical))
            mask = {}
            for i, g in enumerate(G):
                for x in g:
                    mask[x] = mask.get(x, 0) | 1 << i
            best = None
            for (fname, _), g in zip(universe, G):
                sh = len(Q & g)
                jac = ratio(sh, len(g) + len(Q) - sh)
                rows.append([sname, k, fname, len(g), len(Q), sh, ratio(sh, len(g)), ratio(sh, len(Q)), jac])
                if sh and (best is None or jac > best[1]):
                    best = (fname, jac, ratio(sh, len(g)))
            in_pan = sum(1 for x in Q if x in mask)
            in_core = sum(1 for x in Q if mask.get(x) == full)
            summary.append([sname, k, len(Q), in_pan, len(Q) - in_pan, in_core, *(best or (None, None, None))])
            for label, members in groups or []:
                M = sum(1 << i for i in members)
                for cls, (a, b) in zip(CLASSES, ((M, 0), (0, full ^ M), (M, full ^ M))):
                    marker = {x for x, m in mask.items() if m & a == a and m & b == 0}
                    marks.append([sname, k, label, cls, len(marker), len(marker & Q), ratio(len(marker & Q), len(marker))])
    out = {"screen": rows, "screen_summary": summary}
    if groups:
        out["screen_groups"] = marks
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}


def read_csvs(outdir, prefix="gold_5_kmc"):
    got = {}
    for path in glob.glob(os.path.join(outdir, prefix + ".screen*.csv")):
        name = os.path.basename(path)[len(prefix) + 1:-len(".csv")]
        with open(path, newline="") as f:
            body = list(csv.reader(f))
        assert body[0] == COLS[name], name
        got[name] = body[1:]
    return got


class ScreenBackend(cpur.RegionBackend):
    """test_core_regions.RegionBackend with screen_counts from Python sets; card answers the samples' own counts too."""
    name = "exact+core+regions+screen"

    def card(self, path):
        s = json.load(open(path))
        return float(pyref.exact_count([text_of(f) for f in s["fastas"]], int(s["k"]), self.canonical))

    def screen_counts(self, leaf_paths, k, sample_files, all_masks, none_masks):
        n, per_k = self._masks("screen_counts", leaf_paths)
        assert len(per_k) == 1 and int(json.load(open(leaf_paths[0][0]))["k"]) == int(k)
        masks = per_k[0]
        sets = [set(pyref.kmers(text_of(f), int(k), self.canonical)) for f in sample_files] + [set(masks)]
        shared = [[sum(1 for x in q if masks.get(x, 0) >> i & 1) for i in range(n)] for q in sets]
        match = [[sum(1 for x in q if x in masks and masks[x] & int(a) == int(a) and masks[x] & int(b) == 0)
                  for a, b in zip(all_masks, none_masks)] for q in sets]
        return np.array(shared, dtype=np.uint64).reshape(len(sets), n), np.array(match, dtype=np.uint64).reshape(len(sets), len(all_masks))


class NoScreenMasks(ScreenBackend):
    name = "exact+noscreen"

    def screen_counts(self, leaf_paths, k, sample_files, all_masks, none_masks):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def _screen(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["screen", *argv])


def make_samples(tmp_path, data):
    """-> {name: path}: a leaf byte for byte, a relative of a leaf with a novel tail, one that shares nothing, an empty one"""
    d = tmp_path / "samples"
    d.mkdir()
    rng = np.random.default_rng(1019)
    g2 = b"".join(pyref.records(open(os.path.join(data, "g2.fasta"), "rb").read())).decode()
    rel = list(g2[:1500])
    for p in rng.choice(len(rel), size=30, replace=False):
        rel[p] = "ACGT"[("ACGT".index(rel[p].upper()) + 1) % 4] if rel[p].upper() in "ACGT" else "A"
    novel = "".join(rng.choice(list("ACGT"), size=400))
    out = {"leaf": str(d / "leaf.fa"), "rel": str(d / "rel.fa"), "far": str(d / "far.fa"), "none": str(d / "none.fa")}
    shutil.copy(os.path.join(data, "g1.fasta"), out["leaf"])
    with open(out["rel"], "w") as f:
        f.write(">rel one\n" + "".join(rel) + "\n>rel two\n" + novel[:200] + "N" + novel[200:] + "\n")
    with open(out["far"], "w") as f:
        f.write(">far\n" + "AC" * 12 + "\n")
    open(out["none"], "w").close()
    return out


def test_csvs_equal_the_tables_from_the_text(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    s = make_samples(tmp_path, data)
    qlist = tmp_path / "q.txt"
    qlist.write_text(f"{s['rel']}\n{s['leaf']}\n\n{s['far']}\n{s['none']}\n")
    out = str(tmp_path / "o")
    ks = [9, 12]
    ScreenBackend.reset()
    # a positional sample and a -q list, `leaf` in both: listed once, at its first place
    _screen(host, ScreenBackend, ["-d", pk, "-g", gfile, "-k", "12", "-k", "9", "-o", out, "-q", str(qlist), s["leaf"]])
    assert ScreenBackend.calls == {"screen_counts": len(ks)}                # once per k: four samples are one batch
    order = [s["leaf"], s["rel"], s["far"], s["none"]]
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    want = tables(universe, [(p, text_of(p)) for p in order], ks, groups)
    got = read_csvs(out)
    assert sorted(got) == ["screen", "screen_groups", "screen_summary"]
    for name in want:
        assert got[name] == want[name], name
    assert len(got["screen"]) == 4 * 2 * 5 and len(got["screen_summary"]) == 4 * 2 and len(got["screen_groups"]) == 4 * 2 * 3 * 3
    summary = {(r[0], int(r[1])): r for r in got["screen_summary"]}
    table = {(r[0], int(r[1]), os.path.basename(r[2])): r for r in got["screen"]}
    for k in ks:
        # a sample that is a leaf: jaccard 1 with itself, nothing novel
        assert table[(s["leaf"], k, "g1.fasta")][6:] == ["1.0", "1.0", "1.0"]
        assert summary[(s["leaf"], k)][4] == "0" and os.path.basename(summary[(s["leaf"], k)][6]) == "g1.fasta"
        # a sample that shares nothing: no best genome
        assert summary[(s["far"], k)][3] == "0" and summary[(s["far"], k)][6:] == ["", "", ""]
        # an empty sample: no k-mers, the ratios over them are empty cells
        assert summary[(s["none"], k)][2:] == ["0", "0", "0", "0", "", "", ""]
        for name in cpuc.NAMES:
            assert table[(s["none"], k, name)][4:] == ["0", "0", "0.0", "", "0.0"]
        # a relative: closest to where it came from, and something novel
        assert os.path.basename(summary[(s["rel"], k)][6]) == "g2.fasta" and int(summary[(s["rel"], k)][4]) > 0
    # without -g: no groups file; the default k is the root's
    out2 = str(tmp_path / "o2")
    ScreenBackend.reset()
    _screen(host, ScreenBackend, ["-d", pk, "-o", out2, s["rel"]])
    from dandd_amd.host.compat import load_tree
    root_k = int(load_tree(pk).root_k())
    got = read_csvs(out2)
    assert sorted(got) == ["screen", "screen_summary"] and ScreenBackend.calls == {"screen_counts": 1}
    assert got == tables(universe, [(s["rel"], text_of(s["rel"]))], [root_k], None)


def test_samples_go_in_batches(host, tmp_path, monkeypatch):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = make_samples(tmp_path, data)
    order = [s["rel"], s["none"], s["leaf"], s["far"]]
    universe = [(os.path.join(data, name), open(os.path.join(data, name), "rb").read()) for name in cpuc.NAMES]
    want = tables(universe, [(p, text_of(p)) for p in order], [10], None)
    for files, nbytes, calls in ((3, 1 << 40, 2), (64, os.path.getsize(s["rel"]) + 1, 3)):
        monkeypatch.setattr(host.DeltaTree, "SCREEN_BATCH_FILES", files)
        monkeypatch.setattr(host.DeltaTree, "SCREEN_BATCH_BYTES", nbytes)
        out = str(tmp_path / f"b{files}")
        ScreenBackend.reset()
        _screen(host, ScreenBackend, ["-d", pk, "-k", "10", "-o", out, *order])
        assert ScreenBackend.calls == {"screen_counts": calls}
        assert read_csvs(out) == want


def test_exits(host, tmp_path):
    import test_deltadelta as dd
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    s = make_samples(tmp_path, data)
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            _screen(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("screen: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*screen*"))
    fails(ScreenBackend, ["-d", pk, "-k", "0", s["rel"]], "-k 0", "1..64")
    fails(ScreenBackend, ["-d", pk, "-k", "65", s["rel"]], "-k 65", "1..64")
    fails(ScreenBackend, ["-d", pk, s["rel"], str(tmp_path / "nowhere.fa")], "nowhere.fa", "not found")
    fails(ScreenBackend, ["-d", pk], "no sample")
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    fails(ScreenBackend, ["-d", pk, "-q", str(empty)], "no sample")
    fails(cpur.RegionBackend, ["-d", pk, s["rel"]], "screen_counts", "exact membership masks")
    fails(NoScreenMasks, ["-d", pk, s["rel"]], "no membership masks")
    # a tree of sketches: the message `core` gives
    sk = tmp_path / "sk"
    sk.mkdir()
    _, pks = dd._tree(str(sk), host)
    fails(ScreenBackend, ["-d", pks, s["rel"]], "tree --exact", "inclusion-exclusion")
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
    fails(ScreenBackend, ["-d", pk65, s["rel"]], "65 genomes", "at most 64", "-f")


def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_exact_screen", "dd_exact_screen_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dandd_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert hasattr(engine.Engine, "exact_screen") and hasattr(engine.Engine, "exact_screen_device")
    assert engine.Engine.last_screen_found is None
    assert hasattr(HipExactBackend, "screen_counts") and hasattr(DeltaTree, "screen_tables")
