"""`dandd core --kmers` on the CPU: the FASTA files of marker k-mers and their index on the golden exact tree, from a checker
backend that builds the membership masks from Python sets of pyref.kmers (test_core.CoreBackend plus select_kmers); every
sequence, its order and its ngen are compared with the same sets, the index with core_groups.csv, the default k with
core_groupsummary.csv, and the command's exits are checked.  engine.kmer_text is checked against a decode of pyref.kmers
values.  The GPU's records are compared with the same masks in test_gpu_core_kmers.py."""
import glob
import json
import os

import numpy as np
import pytest

import hostcheck
import pyref
import test_core as cpuc
import test_exact_schedules as ex

M64 = (1 << 64) - 1
CLASSES = ("core", "private", "signature")


def records_of(masks, queries):
    """the (k-mer, mask) of {k-mer: mask} that match at least one (all, none) of `queries`, ascending"""
    return sorted((x, m) for x, m in masks.items() if any(m & a == a and m & b == 0 for a, b in queries))


def arrays_of(recs):
    """sorted [(k-mer, mask)] -> (uint64 [m][2] (lo, hi), uint64 [m]), the layout of dd_exact_select_kmers"""
    kmers = np.array([[x & M64, x >> 64] for x, _ in recs], dtype=np.uint64).reshape(-1, 2)
    return kmers, np.array([m for _, m in recs], dtype=np.uint64)


def text_of(x, k):
    return "".join("ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))


class KmerBackend(cpuc.CoreBackend):
    """test_core.CoreBackend with the k-mers behind select_counts, from the same Python sets."""
    name = "exact+core+kmers"

    def select_kmers(self, leaf_paths, k, all_masks, none_masks, limit):
        n, per_k = self._masks("select_kmers", leaf_paths)
        k0 = int(json.load(open(leaf_paths[0][0]))["k"])
        recs = records_of(per_k[int(k) - k0], [(int(a), int(b)) for a, b in zip(all_masks, none_masks)])
        if len(recs) > limit:
            raise ValueError(f"{len(recs)} k-mers match at k={k}, more than the limit of {limit}")
        return arrays_of(recs)


class NoKmerMasks(KmerBackend):
    """the entry point, and no table for these leaves (HipExactBackend above 64 of them)"""
    name = "exact+nokmers"

    def select_kmers(self, leaf_paths, k, all_masks, none_masks, limit):
        return None


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def read_fasta(path):
    """-> [(header without '>', sequence)]"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    assert all(h.startswith(">") for h in lines[:-1:2])
    return [(h[1:], s) for h, s in zip(lines[:-1:2], lines[1:-1:2])]


def query_of(cls, G, full):
    return {"core": (G, 0), "private": (0, full ^ G), "signature": (G, full ^ G)}[cls]


def test_fasta_files_equal_the_set_computation(host, tmp_path):
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    pickle_path = os.path.join(str(tmp_path), "t", "sketchdb", "gold_5_orderings.pickle")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    base = ["-d", pk, "-r", pickle_path, "-g", gfile, *cpuc.WINDOW]
    cpuc._core(host, cpuc.CoreBackend, [*base, "-o", plain])
    KmerBackend.reset()
    cpuc._core(host, KmerBackend, [*base, "-o", out, "--kmers", "core", "--kmers", "signature", "--kmers", "private"])
    # the tables of the parent are what they were, byte for byte; one select_kmers call per distinct k
    before, after = cpuc._outputs(plain), cpuc._outputs(out)
    assert sorted(before) == sorted(f"gold_5_kmc.core_{x}.csv" for x in ("spectrum", "growth", "growthsummary", "groups", "groupsummary"))
    assert {name: text for name, text in after.items() if "core_kmers" not in name} == before
    prefix = os.path.join(out, "gold_5_kmc")
    summary = {r["group"]: r for r in cpuc._rows(prefix + ".core_groupsummary.csv")}
    cells = {(r["group"], int(r["k"])): r for r in cpuc._rows(prefix + ".core_groups.csv")}
    index = cpuc._rows(prefix + ".core_kmers.csv")
    assert list(index[0]) == ["group", "class", "k", "kmers", "file"]
    assert [(r["group"], r["class"]) for r in index] == [(label, c) for label, _ in groups for c in CLASSES]
    assert KmerBackend.calls["select_kmers"] == len({int(r["k"]) for r in index})
    assert sorted(n for n in after if n.endswith(".fasta")) == sorted(r["file"] for r in index)
    want = cpuc._golden(data)
    for r in index:
        gi = [label for label, _ in groups].index(r["group"])
        members = groups[gi][1]
        G, k, cls = sum(1 << i for i in members), int(r["k"]), r["class"]
        assert k == int(summary[r["group"]][f"{cls}_k"])                      # the default k: the summary's argmax
        assert r["file"] == f"gold_5_kmc.core_kmers.g{gi + 1}.{cls}.k{k}.fasta"
        assert int(r["kmers"]) == int(cells[(r["group"], k)][cls])
        recs = records_of(want[k], [query_of(cls, G, 31)])
        got = read_fasta(os.path.join(out, r["file"]))
        assert len(got) == int(r["kmers"]) == len(recs)
        assert [s for _, s in got] == [text_of(x, k) for x, _ in recs]       # the set AND the order: ascending = alphabetical
        assert [s for _, s in got] == sorted(s for _, s in got)
        assert [h for h, _ in got] == [f"{r['group']}.{cls}.k{k}.{j} ngen={bin(m).count('1')}" for j, (_, m) in enumerate(recs, 1)]
    # a single genome's private k-mers and signature are the same list
    alone = {r["class"]: r for r in index if r["group"] == "alone"}
    if alone["private"]["k"] == alone["signature"]["k"]:
        assert [s for _, s in read_fasta(os.path.join(out, alone["private"]["file"]))] == \
               [s for _, s in read_fasta(os.path.join(out, alone["signature"]["file"]))]


def test_exits_and_flags(host, tmp_path):
    import test_deltadelta as dd
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    want = cpuc._golden(data)
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            cpuc._core(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("core: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*.core_*")) and not glob.glob(os.path.join(str(e), "*.fasta"))
    # --kmers-k: at the given k, whatever the argmax; outside the window an exit
    out = str(tmp_path / "k")
    cpuc._core(host, KmerBackend, ["-d", pk, "-o", out, "-g", gfile, *cpuc.WINDOW, "--kmers", "signature", "--kmers-k", "8", "--kmers-k", "12"])
    index = cpuc._rows(os.path.join(out, "gold_5_kmc.core_kmers.csv"))
    assert [(r["group"], r["class"], int(r["k"])) for r in index] == [(label, "signature", k) for label, _ in groups for k in (8, 12)]
    for r in index:
        G = sum(1 << i for i in dict(groups)[r["group"]])
        recs = records_of(want[int(r["k"])], [(G, 31 ^ G)])
        assert [s for _, s in read_fasta(os.path.join(out, r["file"]))] == [text_of(x, int(r["k"])) for x, _ in recs]
    fails(KmerBackend, ["-d", pk, "-g", gfile, *cpuc.WINDOW, "--kmers", "core", "--kmers-k", "13"], "--kmers-k 13", "8..12")
    fails(KmerBackend, ["-d", pk, "-g", gfile, *cpuc.WINDOW, "--kmers", "core", "--kmers-k", "7"], "--kmers-k 7", "8..12")
    # --kmers-max: the count, the advice, nothing written
    left_core = {k: cpuc.select_of(want[k], 5, 0) for k in cpuc.KS}
    kbest = cpuc._delta([left_core[k] for k in cpuc.KS], cpuc.KS)[1]
    assert left_core[kbest] > 3
    fails(KmerBackend, ["-d", pk, "-g", gfile, *cpuc.WINDOW, "--kmers", "core", "--kmers-max", "3"], f"{left_core[kbest]} k-mers", "--kmers-max 3", "raise it", "narrow")
    # a backend without select_kmers / without masks for these leaves, as for the tables
    fails(cpuc.CoreBackend, ["-d", pk, "-g", gfile, *cpuc.WINDOW, "--kmers", "core"], "select_kmers", "exact membership masks")
    fails(NoKmerMasks, ["-d", pk, "-g", gfile, *cpuc.WINDOW, "--kmers", "core"], "no membership masks")
    fails(cpuc.NoMasks, ["-d", pk, *cpuc.WINDOW, "--kmers", "core"], "no membership masks")
    # a tree of sketches
    sk = tmp_path / "sk"
    sk.mkdir()
    _, pks = dd._tree(str(sk), host)
    fails(KmerBackend, ["-d", pks, *cpuc.WINDOW, "--kmers", "core"], "tree --exact", "inclusion-exclusion")
    # no -g: one implied group `all`, the whole universe; its core is the core genome, its private k-mers every k-mer
    out = str(tmp_path / "all")
    cpuc._core(host, KmerBackend, ["-d", pk, "-o", out, *cpuc.WINDOW, "--kmers", "core", "--kmers", "private", "--kmers-k", "9"])
    index = cpuc._rows(os.path.join(out, "gold_5_kmc.core_kmers.csv"))
    assert [(r["group"], r["class"], int(r["k"]), r["file"]) for r in index] == \
        [("all", c, 9, f"gold_5_kmc.core_kmers.g1.{c}.k9.fasta") for c in ("core", "private")]
    got = read_fasta(os.path.join(out, index[0]["file"]))
    assert [s for _, s in got] == [text_of(x, 9) for x, m in sorted(want[9].items()) if m == 31] and got
    assert all(h.endswith(" ngen=5") for h, _ in got)
    assert [s for _, s in read_fasta(os.path.join(out, index[1]["file"]))] == [text_of(x, 9) for x in sorted(want[9])]
    assert int(index[1]["kmers"]) == pyref.exact_count([open(os.path.join(data, n), "rb").read() for n in cpuc.NAMES], 9)


def test_kmer_text_decodes_both_words():
    from dandd_amd import engine
    rng = np.random.default_rng(64)
    for k in (1, 2, 31, 32, 33, 63, 64):
        seqs = ["".join(rng.choice(list("ACGT"), size=k)) for _ in range(40)] + ["A" * k, "T" * k, "G" + "A" * (k - 1), "T" + "C" * (k - 1)]
        vals = []
        for s in seqs:
            got = pyref.kmers((">s\n" + s + "\n").encode(), k, canonical=False)
            assert len(got) == 1
            vals.append(got[0])
        kmers, _ = arrays_of([(x, 0) for x in vals])
        assert engine.kmer_text(kmers, k) == seqs == [text_of(x, k) for x in vals]
        if k in (32, 64):                                           # G.. / T..: the top bit of the most significant word
            assert int(kmers[-2, k // 64]) >> 63 == 1 and int(kmers[-1, k // 64]) >> 63 == 1
        if k == 64:
            assert any(int(lo) >> 63 for lo in kmers[:, 0]) and any(int(hi) >> 63 for hi in kmers[:, 1])
    assert engine.kmer_text(np.zeros((0, 2), dtype=np.uint64), 21) == []
    with pytest.raises(ValueError):
        engine.kmer_text(np.zeros((1, 2), dtype=np.uint64), 65)


def test_binding_and_backend_have_the_entry_points():
    from dandd_amd import engine
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    assert hasattr(engine.Engine, "exact_select_kmers") and hasattr(engine.Engine, "exact_select_kmers_device")
    assert "dd_exact_select_kmers" in engine.EXPORTS and "dd_exact_select_kmers_device" in engine.EXPORTS
    assert hasattr(HipExactBackend, "select_kmers") and hasattr(DeltaTree, "core_kmers")
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and hasattr(lib, "dd_exact_select_kmers") and hasattr(lib, "dd_exact_select_kmers_device")
