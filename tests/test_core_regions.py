"""`dandd core --regions` on the CPU: the record index of the host library (engine.fasta_index) against a table derived from
pyref.records, on the fixture genomes the GPU tests share (below) and their .gz copies; engine.regions_from_hits on hand-made
bitmaps; and the command on the golden exact tree with a checker backend that paints positions from Python sets
(test_core_kmers.KmerBackend plus locate_hits): every BED file against a brute-force per-base coverage computed from the same
sets, the index CSV, and the command's exits.  The GPU's bitmaps are compared with the same reference in
test_gpu_core_regions.py."""
import functools
import glob
import gzip
import json
import os

import numpy as np
import pytest

import pyref
import test_core as cpuc
import test_core_kmers as cpuk
import test_exact_schedules as ex

CLASSES = ("core", "private", "signature")


# ---- the fixture the CPU and GPU tests share -----------------------------------------------------------------------------
# A seeded ancestor of 6 kbp, 2 % substitutions per genome.  g1 / g2 are cut so that their token streams (one BREAK for the
# record, then the bases) are 64 m and 64 m + 1 tokens long; g3 has three records: an empty one, one with a run of 30 N, a
# lowercase stretch, \r\n line ends and runs of 70 T and 70 A (T^k is the all-ones key), and a plain one; g4 is g0 byte for
# byte; g5 is one record of 40 bases (shorter than most k); g6 is an empty file.
GROUPS = [[0, 4], [1, 2], [3]]
NAMES = [["g0"], ["g1"], ["g2"], ["g3_empty", "g3_odd", "g3_plain"], ["g0"], ["g5"], []]


@functools.lru_cache(maxsize=None)
def genomes():
    rng = np.random.default_rng(20261019)
    anc = rng.integers(0, 4, 6100)

    def mutant(length):
        s = anc[:length].copy()
        mut = rng.random(length) < 0.02
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        return "".join("ACGT"[c] for c in s)

    def lines(t, width=70, eol="\n"):
        return "".join(t[j:j + width] + eol for j in range(0, len(t), width))
    g0 = (">g0 the first\n" + lines(mutant(6000))).encode()
    g1 = (">g1\n" + lines(mutant(64 * 94 - 1))).encode()
    g2 = (">g2\tx\n" + lines(mutant(64 * 94), 61)).encode()
    t = mutant(6000)
    odd = t[:900] + "N" * 30 + t[900:1500].lower() + "T" * 70 + t[1500:2400] + "A" * 70 + t[2400:3000] + "R" + t[3000:3100]
    g3 = (">g3_empty nothing here\r\n>g3_odd\r\n" + lines(odd, 70, "\r\n") + ">g3_plain z\n" + lines(t[3100:])).encode()
    g5 = (">g5\n" + mutant(40) + "\n").encode()
    return (g0, g1, g2, g3, g0, g5, b"")


def write_genomes(tmp_path):
    paths = []
    for i, fa in enumerate(genomes()):
        p = str(tmp_path / f"g{i}.fa")
        with open(p, "wb") as fh:
            fh.write(fa)
        paths.append(p)
    return paths


def index_of(fa):
    """(seq_len, tok_start, ntok) of a buffer in K0's layout -- one BREAK in front of every record's bases -- from pyref.records"""
    lens = [len(s) for s in pyref.records(fa)]
    starts, at = [], 0
    for n in lens:
        starts.append(at + 1)
        at += 1 + n
    return lens, starts, at


def tokens_of(fa):
    toks = []
    for seq in pyref.records(fa):
        toks.append(4)
        toks.extend(pyref.CODE.get(c, 4) for c in seq)
    return toks


def ends_of(fa, k, canonical):
    """{token index: (canonical) k-mer that ENDS there} -- pyref.kmers' window rule with rolling words"""
    out, run, f, r = {}, 0, 0, 0
    full = (1 << 2 * k) - 1
    for t, c in enumerate(tokens_of(fa)):
        if c == 4:
            run = f = r = 0
            continue
        run += 1
        f = ((f << 2) | c) & full
        r = (r >> 2) | ((3 - c) << 2 * (k - 1))
        if run >= k:
            out[t] = min(f, r) if canonical else f
    return out


@functools.lru_cache(maxsize=None)
def reference(k, canonical):
    """-> ([{end token: key}] per genome, {key: membership mask}) of the fixture"""
    ends = [ends_of(fa, k, canonical) for fa in genomes()]
    masks = {}
    for i, e in enumerate(ends):
        for x in e.values():
            masks[x] = masks.get(x, 0) | 1 << i
    return ends, masks


def bitmap(tokens, ntok):
    w = np.zeros((ntok + 63) // 64, dtype=np.uint64)
    for t in tokens:
        w[t // 64] |= np.uint64(1 << (t % 64))
    return w


def want_bitmap(k, canonical, a, b, g):
    ends, masks = reference(k, canonical)
    ntok = index_of(genomes()[g])[2]
    return bitmap([t for t, x in ends[g].items() if masks[x] & a == a and masks[x] & b == 0], ntok)


def group_jobs(n=7, groups=GROUPS):
    """3 classes x the groups x each group's genomes: (all, none, genome)"""
    full = (1 << n) - 1
    jobs = []
    for members in groups:
        G = sum(1 << i for i in members)
        for a, b in ((G, 0), (0, full ^ G), (G, full ^ G)):
            jobs.extend((a, b, g) for g in members)
    return jobs


# ---- 1. the record index ------------------------------------------------------------------------------------------------
def same_index(got, names, fa):
    lens, starts, ntok = index_of(fa)
    assert got[0] == names
    assert got[1].dtype == np.uint64 and got[2].dtype == np.uint64
    assert got[1].tolist() == lens and got[2].tolist() == starts and got[3] == ntok


def test_fasta_index_equals_the_records_of_pyref(tmp_path):
    from dandd_amd import engine
    paths = write_genomes(tmp_path)
    fas = genomes()
    assert index_of(fas[1])[2] % 64 == 0 and index_of(fas[2])[2] % 64 == 1
    for p, fa, names in zip(paths, fas, NAMES):
        same_index(engine.fasta_index(p), names, fa)
        with open(p + ".gz", "wb") as fh:
            fh.write(gzip.compress(fa))
        same_index(engine.fasta_index(p + ".gz"), names, fa)
    # text in front of the first header, an empty record, a '>' inside a line, a header the end of the buffer cuts short
    odd = b"junk\n>r1 first\nACGTNNAC\r\nacgt\r\n>e\n>r3\tx\nAC>GT\nTTTT\n>cut"
    (tmp_path / "odd.fa").write_bytes(odd)
    same_index(engine.fasta_index(str(tmp_path / "odd.fa")), ["r1", "e", "r3", "cut"], odd)
    # FASTQ: the names survive the rewrite into FASTA; the record cut off in its quality text is dropped
    fq = b"@q1 x\nACGT\n+\nIIII\n@q2\nGGN\n+q2\nIII\n@q3\nAC\n+\nI"
    (tmp_path / "r.fq").write_bytes(fq)
    assert len(pyref.records(fq)) == 2
    same_index(engine.fasta_index(str(tmp_path / "r.fq")), ["q1", "q2"], fq)
    # more records than the first call has room for
    many = "".join(f">n{i}\nAC\n" for i in range(3000)).encode()
    (tmp_path / "many.fa").write_bytes(many)
    same_index(engine.fasta_index(str(tmp_path / "many.fa")), [f"n{i}" for i in range(3000)], many)
    with pytest.raises(engine.EngineError, match="nowhere.fa"):
        engine.fasta_index(str(tmp_path / "nowhere.fa"))


# ---- 2. bitmaps -> intervals ----------------------------------------------------------------------------------------------
def test_regions_from_hits_on_hand_made_bitmaps():
    from dandd_amd.engine import regions_from_hits
    k = 7
    tok_start, seq_len = [1, 102, 103], [100, 0, 200]        # record 1 is empty; ntok = 303

    def spans(*tokens):
        return [r.tolist() for r in regions_from_hits(bitmap(tokens, 303), k, tok_start, seq_len)]
    assert spans() == [[], [], []]
    assert spans(1 + k - 1) == [[[0, k]], [], []]                                       # a hit at start + k - 1: [0, k)
    assert spans(20, 20 + k) == [[[20 - k, 20 + k]], [], []]                            # k apart: abutting, one interval
    assert spans(20, 20 + k + 1) == [[[20 - k, 20], [21, 21 + k]], [], []]              # k + 1 apart: a base between them
    assert spans(20, 21, 22, 40) == [[[20 - k, 22], [40 - k, 40]], [], []]
    assert spans(100, 103 + k - 1) == [[[100 - k, 100]], [], [[0, k]]]                  # the last k-mer of record 0, the first of 2:
    assert spans(63, 64) == [[[63 - k, 64]], [], []]                                    # ... never one interval; bits 63 | 64 are
    assert spans(127, 128) == [[], [], [[127 - 103 + 1 - k, 128 - 103 + 1]]]           # neighbours across words
    got = regions_from_hits(bitmap([302], 303), k, tok_start, seq_len)
    assert got[2].tolist() == [[200 - k, 200]] and got[2].dtype == np.int64 and got[0].shape == (0, 2)
    for bad in (1 + k - 2, 101, 102):        # a k-mer that would start in front of its record; the BREAKs of records 1 and 2
        with pytest.raises(ValueError):
            regions_from_hits(bitmap([bad], 303), k, tok_start, seq_len)
    assert [r.tolist() for r in regions_from_hits(np.zeros(0, dtype=np.uint64), k, [], [])] == []


# ---- 3. the command --------------------------------------------------------------------------------------------------------
def header_names(fa):
    return [line[1:].split()[0].decode() if line[1:].split() else "" for line in fa.split(b"\n") if line[:1] == b">"]


class RegionBackend(cpuk.KmerBackend):
    """test_core_kmers.KmerBackend with the positions behind select_kmers, from the same Python sets."""
    name = "exact+core+regions"

    def locate_hits(self, leaf_paths, k, jobs):
        n, per_k = self._masks("locate_hits", leaf_paths)
        k0 = int(json.load(open(leaf_paths[0][0]))["k"])
        masks = per_k[int(k) - k0]
        fas = [open(json.load(open(row[0]))["fastas"][0], "rb").read() for row in leaf_paths]
        index = []
        for fa in fas:
            lens, starts, ntok = index_of(fa)
            index.append((header_names(fa), np.array(lens, dtype=np.uint64), np.array(starts, dtype=np.uint64), ntok))
        ends = [ends_of(fa, int(k), self.canonical) for fa in fas]
        hits = [bitmap([t for t, x in ends[g].items() if masks[x] & a == a and masks[x] & b == 0], index[g][3]) for a, b, g in jobs]
        return index, hits


class NoRegionMasks(RegionBackend):
    name = "exact+noregions"

    def locate_hits(self, leaf_paths, k, jobs):
        return None


def coverage_rows(fa, k, masks, a, b):
    """[(record name, start, end)]: maximal runs of the bases covered by a k-mer whose mask matches (a, b) -- per base, from
    the record's text and the {k-mer: mask} of the universe, no token stream and no bitmap"""
    rows = []
    for name, seq in zip(header_names(fa), pyref.records(fa)):
        codes = [pyref.CODE.get(c, 4) for c in seq]
        covered = [False] * len(seq)
        for p in range(len(seq) - k + 1):
            w = codes[p:p + k]
            if 4 in w:
                continue
            f = r = 0
            for c in w:
                f = (f << 2) | c
            for c in reversed(w):
                r = (r << 2) | (3 - c)
            m = masks[min(f, r)]
            if m & a == a and m & b == 0:
                covered[p:p + k] = [True] * k
        p = 0
        while p < len(seq):
            if covered[p]:
                q = p
                while q < len(seq) and covered[q]:
                    q += 1
                rows.append((name, p, q))
                p = q
            else:
                p += 1
    return rows


def check_outputs(out, data, groups, ks_of):
    """every file `core --regions` wrote under `out` against coverage_rows; ks_of(label, cls) -> the ks expected"""
    prefix = os.path.join(out, "gold_5_kmc")
    want = cpuc._golden(data)
    index = cpuc._rows(prefix + ".core_regions.csv")
    assert list(index[0]) == ["group", "class", "k", "fasta", "regions", "bases", "file"]
    expect = [(label, c, k, cpuc.NAMES[g]) for label, members in groups for c in CLASSES if ks_of(label, c)
              for k in ks_of(label, c) for g in sorted(members)]
    assert [(r["group"], r["class"], int(r["k"]), r["fasta"]) for r in index] == expect
    files = sorted({r["file"] for r in index})
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "*.bed"))) == files
    n = len(cpuc.NAMES)
    for name in files:
        mine = [r for r in index if r["file"] == name]
        label, cls, k = mine[0]["group"], mine[0]["class"], int(mine[0]["k"])
        gi = [lab for lab, _ in groups].index(label)
        assert name == f"gold_5_kmc.core_regions.g{gi + 1}.{cls}.k{k}.bed"
        G = sum(1 << i for i in groups[gi][1])
        a, b = cpuk.query_of(cls, G, (1 << n) - 1)
        lines = []
        for r, g in zip(mine, sorted(groups[gi][1])):
            rows = coverage_rows(open(os.path.join(data, cpuc.NAMES[g]), "rb").read(), k, want[k], a, b)
            assert (int(r["regions"]), int(r["bases"])) == (len(rows), sum(e - s for _, s, e in rows)), r
            lines.extend(f"{rec}\t{s}\t{e}\t{cpuc.NAMES[g]}\n" for rec, s, e in rows)
        assert open(os.path.join(out, name)).read() == "".join(lines), name
    return index


def test_bed_files_equal_the_per_base_coverage(cpuk_host, tmp_path):
    host = cpuk_host
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, groups = cpuc._groups_file(tmp_path, data)
    plain, out = str(tmp_path / "plain"), str(tmp_path / "o")
    base = ["-d", pk, "-g", gfile, *cpuc.WINDOW]
    cpuc._core(host, cpuc.CoreBackend, [*base, "-o", plain])
    RegionBackend.reset()
    cpuc._core(host, RegionBackend, [*base, "-o", out, "--regions", "private", "--regions", "core", "--regions", "signature"])
    # the tables of the parent are what they were, byte for byte; one locate_hits call per distinct k
    before, after = cpuc._outputs(plain), cpuc._outputs(out)
    assert {name: text for name, text in after.items() if "core_regions" not in name} == before
    summary = {r["group"]: r for r in cpuc._rows(os.path.join(out, "gold_5_kmc.core_groupsummary.csv"))}
    index = check_outputs(out, data, groups, lambda label, cls: [int(summary[label][f"{cls}_k"])])
    assert RegionBackend.calls["locate_hits"] == len({int(r["k"]) for r in index})
    assert len(index) == 3 * 5 and any(int(r["regions"]) > 1 for r in index)
    # --regions-k: at the given ks, whatever the argmax, next to --kmers
    out = str(tmp_path / "k")
    cpuc._core(host, RegionBackend, [*base, "-o", out, "--regions", "signature", "--regions-k", "12", "--regions-k", "8", "--kmers", "core"])
    check_outputs(out, data, groups, lambda label, cls: [8, 12] if cls == "signature" else [])
    assert os.path.exists(os.path.join(out, "gold_5_kmc.core_kmers.csv"))
    # no -g: one implied group `all`; its private k-mers are every k-mer, so every base a k-mer covers is painted
    out = str(tmp_path / "all")
    cpuc._core(host, RegionBackend, ["-d", pk, *cpuc.WINDOW, "-o", out, "--regions", "private", "--regions-k", "9"])
    index = check_outputs(out, data, [("all", [0, 1, 2, 3, 4])], lambda label, cls: [9] if cls == "private" else [])
    assert [r["file"] for r in index] == ["gold_5_kmc.core_regions.g1.private.k9.bed"] * 5


@pytest.fixture
def cpuk_host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)
    os.environ.pop("DD_NO_PREFETCH", None)


def test_exits(cpuk_host, tmp_path):
    host = cpuk_host
    pk = ex.exact_tree(str(tmp_path), host)
    data = str(tmp_path / "data")
    gfile, _ = cpuc._groups_file(tmp_path, data)
    e = tmp_path / "e"

    def fails(backend, argv, *texts):
        with pytest.raises(SystemExit) as err:
            cpuc._core(host, backend, [*argv, "-o", str(e)])
        code = err.value.code
        assert isinstance(code, str) and code.startswith("core: ") and "\n" not in code, (argv, code)
        for text in texts:
            assert text in code, (text, code)
        assert not glob.glob(os.path.join(str(e), "*.core_*")) and not glob.glob(os.path.join(str(e), "*.bed"))
    base = ["-d", pk, "-g", gfile, *cpuc.WINDOW]
    fails(RegionBackend, [*base, "--regions-k", "9"], "--regions-k goes with --regions")
    fails(RegionBackend, [*base, "--regions", "core", "--regions-k", "13"], "--regions-k 13", "8..12")
    fails(RegionBackend, [*base, "--regions", "core", "--regions-k", "7"], "--regions-k 7", "8..12")
    fails(cpuk.KmerBackend, [*base, "--regions", "core"], "locate_hits", "exact membership masks")
    fails(NoRegionMasks, [*base, "--regions", "core"], "no membership masks")


def test_binding_and_backend_have_the_entry_points():
    from dandd_amd import engine
    from dandd_amd.host.backend import HipExactBackend
    from dandd_amd.host.deltatree import DeltaTree
    assert hasattr(engine.Engine, "exact_locate") and hasattr(engine.Engine, "exact_locate_device")
    assert {"dd_exact_locate", "dd_exact_locate_device", "dd_fasta_index"} <= set(engine.EXPORTS)
    assert hasattr(HipExactBackend, "locate_hits") and hasattr(DeltaTree, "core_regions")
    lib = engine.load_library()
    assert lib.dd_abi_version() == 4 and all(hasattr(lib, name) for name in ("dd_exact_locate", "dd_exact_locate_device", "dd_fasta_index"))
