"""`dandd neighbors` on the CPU: new samples against a tree of sketches.

The command runs on the oracle backend with an oracle cross_cards; its three files are compared with tests/neighbors_ref.py
fed with cardinalities taken straight from the FASTA files (oracle sketch, numpy maximum, oracle card).  Then its options, the
tree's files before and after, its exits, and the entry points of every layer."""
import csv
import glob
import io
import os
import re
import shutil
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck
import neighbors_ref
import test_deltadelta as dd

LO, HI, REGS = 8, 16, 12
WINDOW = ["--ksweep", "--mink", str(LO), "--maxk", str(HI)]
KS = list(range(LO, HI + 1))


class NeighborsBackend(hostcheck.ScheduleBackend):
    """The schedule backend with what `neighbors` asks of a backend, brute force on the oracle"""
    name = "oracle+cross"

    def sample_sketches(self, files, kmin, kmax):
        return np.array([[self.orc.sketch(np.fromfile(f, dtype=np.uint8), k, self.log2m, self.canonical) for k in range(kmin, kmax + 1)]
                         for f in files])

    def sample_cards(self, regs):
        return np.array([self.orc.card(r, self.log2m) for r in regs])

    def cross_cards(self, sample_regs, leaf_paths, merged=False):
        slab = np.array(self._slab(leaf_paths))
        if merged:
            slab = slab.max(axis=0, keepdims=True)
        return np.array([[[self.orc.card(np.maximum(s[kk], g[kk]), self.log2m) for kk in range(slab.shape[1])] for g in slab] for s in sample_regs])


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)


def make_world(tmp_path, host, registers=REGS):
    """A 5-leaf tree of sketches with a window, and three samples: a copy of leaf g2 under another name, a mutated g0, and
    a sequence of its own"""
    with redirect_stdout(io.StringIO()):
        data, pk = dd._tree(str(tmp_path), host, registers=registers, extra=WINDOW)
    rng = np.random.default_rng(3)
    sdir = tmp_path / "samples"
    sdir.mkdir()
    twin = str(sdir / "twin.fasta")
    shutil.copyfile(os.path.join(data, "g2.fasta"), twin)
    text = bytearray(open(os.path.join(data, "g0.fasta"), "rb").read())
    body = [i for i, c in enumerate(text) if c in b"ACGT" and text[:i].rfind(b">") <= text[:i].rfind(b"\n")]
    for i in rng.choice(body, size=len(body) // 50, replace=False):
        text[i] = b"ACGT"[(b"ACGT".index(text[i]) + 1) % 4]
    cousin = str(sdir / "cousin.fasta")
    open(cousin, "wb").write(bytes(text))
    alone = str(sdir / "alone.fasta")
    open(alone, "wb").write(b">alone\n" + rng.choice(np.frombuffer(b"ACGT", np.uint8), size=6000).tobytes() + b"\n")
    return data, pk, [cousin, twin, alone]


@pytest.fixture
def world(tmp_path, host):
    return make_world(tmp_path, host)


def _neighbors(host, argv, backend=NeighborsBackend):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    with redirect_stdout(io.StringIO()):
        cli.main(["neighbors", *argv])


def _table(path):
    with open(path, newline="") as f:
        got = list(csv.reader(f))
    return got[0], got[1:]


def _same(got, want):
    """csv cells against the restatement's values: text as it is, numbers as the doubles they are"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            if b is None:
                assert a == ""
            elif isinstance(b, str):
                assert a == b
            else:
                assert float(a) == float(b), (g, w)


def _restated(orc, fastas, samples, top=None):
    sk = lambda f: [orc.sketch(np.fromfile(f, dtype=np.uint8), k, REGS, True) for k in KS]
    card = lambda rows: [orc.card(r, REGS) for r in rows]
    G, S = [sk(f) for f in fastas], [sk(f) for f in samples]
    U = [np.maximum.reduce([g[kk] for g in G]) for kk in range(len(KS))]
    return neighbors_ref.rows(samples, fastas, KS, [card(s) for s in S], [card(g) for g in G],
                              [[card([np.maximum(a, b) for a, b in zip(s, g)]) for g in G] for s in S], card(U),
                              [card([np.maximum(a, b) for a, b in zip(s, U)]) for s in S], top)


def _tree_files(pk):
    sketchdb = os.path.join(os.path.dirname(pk), "sketchdb")
    listing = sorted(os.path.relpath(os.path.join(d, f), sketchdb) for d, _, fs in os.walk(sketchdb) for f in fs)
    cardkeys = glob.glob(os.path.join(sketchdb, "*cardinalities*"))
    assert cardkeys
    return open(pk, "rb").read(), {c: open(c, "rb").read() for c in cardkeys}, listing


def test_command_against_the_restatement(host, world, orc, tmp_path):
    data, pk, samples = world
    fastas = [os.path.join(data, n) for n in dd.NAMES]
    before = _tree_files(pk)
    out = str(tmp_path / "n")
    _neighbors(host, ["-d", pk, "-o", out, "--jaccard", *samples])
    assert _tree_files(pk) == before                            # pickle, cardinality cache and sketch directory: untouched
    near, summary, jac = _restated(orc, fastas, samples)
    from dandd_amd.host import cli
    for name, want in (("neighbors", near), ("neighbors_summary", summary), ("neighbors_j", jac)):
        head, got = _table(os.path.join(out, f"gold_5_dashing.{name}.csv"))
        assert head == neighbors_ref.COLS[name] == cli.NEIGHBORS_COLUMNS[name]
        _same(got, want)
    head, got = _table(os.path.join(out, "gold_5_dashing.neighbors.csv"))
    assert len(got) == 15 and len(jac) == 3 * 5 * len(KS)
    for s, sample in enumerate(samples):
        mine = [r for r in got if r[0] == sample]
        assert [int(r[9]) for r in mine] == [1, 2, 3, 4, 5]
        assert all(float(a[8]) >= float(b[8]) for a, b in zip(mine, mine[1:]))
    twin = [r for r in got if r[0] == samples[1]]
    assert os.path.basename(twin[0][1]) == "g2.fasta" and float(twin[0][8]) == 1.0 and int(twin[0][9]) == 1
    assert all(float(r[8]) < 1.0 for r in twin[1:])
    head, rows = _table(os.path.join(out, "gold_5_dashing.neighbors_summary.csv"))
    by = {r[0]: r for r in rows}
    assert os.path.basename(by[samples[1]][3]) == "g2.fasta" and float(by[samples[1]][4]) == 1.0 and float(by[samples[1]][9]) == 0.0
    assert os.path.basename(by[samples[0]][3]) == "g0.fasta" and 0.0 < float(by[samples[0]][4]) < 1.0
    assert float(by[samples[2]][9]) > 0.0                       # a sequence of its own adds to the collection's delta


def test_options(host, world, orc, tmp_path):
    data, pk, samples = world
    before = _tree_files(pk)
    sub = [os.path.join(data, n) for n in ("g3.fasta", "g0.fasta", "g2.fasta")]
    flist, qlist = tmp_path / "sub.txt", tmp_path / "q.txt"
    flist.write_text("".join(f + "\n" for f in sub))
    qlist.write_text("".join(f + "\n" for f in samples[1:]))
    out = str(tmp_path / "o")
    _neighbors(host, ["-d", pk, "-o", out, "-f", str(flist), "-q", str(qlist), "--top", "2", samples[0], "-l", "sub"])
    assert _tree_files(pk) == before
    assert not glob.glob(os.path.join(out, "*neighbors_j*"))
    near, summary, _ = _restated(orc, sub, samples, top=2)       # (positional samples first, then the list's; the subset's own union)
    _same(_table(os.path.join(out, "gold_sub_5_dashing.neighbors.csv"))[1], near)
    _same(_table(os.path.join(out, "gold_sub_5_dashing.neighbors_summary.csv"))[1], summary)
    assert len(near) == 6
    # a sample that is a leaf of the tree is allowed: KIJ 1 with itself
    out2 = str(tmp_path / "o2")
    _neighbors(host, ["-d", pk, "-o", out2, "--top", "1", os.path.join(data, "g4.fasta")])
    (row,) = _table(os.path.join(out2, "gold_5_dashing.neighbors.csv"))[1]
    assert os.path.basename(row[1]) == "g4.fasta" and float(row[8]) == 1.0
    assert _tree_files(pk) == before


def test_exits(host, world, tmp_path):
    data, pk, samples = world
    e = tmp_path / "e"

    def fails(argv, text, backend=NeighborsBackend):
        with pytest.raises(SystemExit) as err:
            _neighbors(host, ["-o", str(e), *argv], backend)
        assert isinstance(err.value.code, str) and text in err.value.code and "\n" not in err.value.code, (argv, err.value.code)
        assert not glob.glob(os.path.join(str(e), "*neighbors*"))
    fails(["-d", pk, str(tmp_path / "nowhere.fasta")], "nowhere.fasta not found")
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    fails(["-d", pk, "-q", str(empty)], "no sample")
    fails(["-d", pk, "-q", str(tmp_path / "nolist.txt")], "(-q) not found")
    fails(["-d", pk, "--top", "0", samples[0]], "--top 0")
    fails(["-d", pk, samples[0]], "has no cross_cards", backend=hostcheck.ScheduleBackend)
    # a tree without a window, and no --ksweep
    plain = tmp_path / "plain"
    plain.mkdir()
    with redirect_stdout(io.StringIO()):
        _, pk2 = dd._tree(str(plain), host, registers=REGS)
    fails(["-d", pk2, samples[0]], "a k window is needed")
    # an exact tree: `screen` is the command for it
    exact = tmp_path / "exact"
    exact.mkdir()
    host.set_backend_factory(lambda r, c: hostcheck.ExactBackend(r, c))
    from dandd_amd.host import cli
    with redirect_stdout(io.StringIO()):
        cli.main(["tree", "-d", data, "-o", str(exact), "-s", "gold", "-k", "10", "--exact"])
    (pk3,) = glob.glob(os.path.join(str(exact), "*dtree.pickle"))
    fails(["-d", pk3, *WINDOW, samples[0]], "`screen`")


def test_every_layer_has_the_entry_points():
    from dandd_amd import build, engine
    from dandd_amd.host import cli
    from dandd_amd.host.backend import HipBackend
    from dandd_amd.host.deltatree import DeltaTree
    names = {"dd_cross", "dd_cross_device", "dd_cross_host_device"}
    assert names <= set(engine.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dandd_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert names <= set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header))
    assert re.search(r"#define\s+DD_K2_CROSS_STREAM\s+5\b", text) and re.search(r"#define\s+DD_K2_CROSS_GRAM\s+6\b", text)
    build.build()
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in names)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    assert names <= {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert all(hasattr(engine.Engine, m) for m in ("cross", "cross_device", "cross_host_device"))
    assert engine.Engine.K2_PATHS[5] == "cross_stream" and engine.Engine.K2_PATHS[6] == "cross_gram"
    assert all(hasattr(HipBackend, m) for m in ("cross_cards", "sample_sketches", "sample_cards")) and hasattr(DeltaTree, "neighbor_tables")
    assert "neighbors" in cli.build_parser()._subparsers._group_actions[0].choices and "neighbors" in cli.__doc__
    args = cli.build_parser().parse_args(["neighbors", "-d", "t.pickle", "--top", "3", "--jaccard", "-q", "list.txt", "s.fa"])
    assert args.top == 3 and args.jaccard is True and args.query_loc == "list.txt" and args.samples == ["s.fa"] and args.ksweep is None
    assert cli.NEIGHBORS_COLUMNS == neighbors_ref.COLS
