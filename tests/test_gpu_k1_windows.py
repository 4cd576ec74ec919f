"""GPU: the K1 kernels' k-mer windows are cut from the token words of halo and segment (dd_k1.h: SegWords, Windows<...>::slice),
whole register slabs against the oracle byte for byte.  What a slice can get wrong is a word or a token position, so the input
puts the places where windows become valid again -- the first clean token behind a BREAK -- at every word edge of a segment:

  genome 0   2 x 65 536 + 77 tokens (two full tiles of 1024 segments and a ragged third).  Single Ns and record boundaries so
             that the first clean token behind them falls at stream positions = 14, 15, 16, 17 (mod 16) in every word of a
             segment, i.e. = 14 .. 17, 30 .. 33, 46 .. 49 and 62, 63, 64, 65 (mod 64), once behind an N and once behind a
             record's BREAK; one run of 70 Ns (a whole segment and its halo of BREAKs); an N as the last token of the first tile;
             plain bases to the end.
  genome 1   50 bases: shorter than one segment, every window reaches into the zero halo of segment 0.

  k ranges   both sides of every class edge (32-, 64-, 96-, 128-bit windows) and the headline's 4 .. 40, canonical and forward.
  log2m 14   sweep_kernel (registers in LDS).
  log2m 17   the record path with every tile an epoch of its own (DD_BUCKET_E0 = DD_BUCKET_EMAX = 1): the first tile goes
             through scatter_first_bin_kernel, the second and third through scatter_kernel."""
import functools
import random

import numpy as np
import pytest

TILE = 65_536
NTOK = 2 * TILE + 77
K_RANGES = [(10, 16), (15, 18), (31, 34), (47, 50), (63, 64), (4, 40)]
EDGES = [14, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 62, 63, 64, 65]   # first clean token behind a BREAK, mod 64


class _Stream:
    """FASTA text whose position in the token stream is known: a header line is one BREAK in front of its record, a base one
    token, an N one BREAK."""

    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.text = []
        self.pos = 0
        self.first_clean = []     # stream positions of the first clean token behind a BREAK that was placed on purpose
        self.rec_starts = []

    def header(self):
        if self.text:
            self.text.append("\n")
        self.text.append(f">r{len(self.rec_starts)}\n")
        self.pos += 1
        self.rec_starts.append(self.pos)

    def bases(self, n):
        self.text.append("".join(self.rnd.choice("ACGT") for _ in range(n)))
        self.pos += n

    def ns(self, n):
        self.text.append("N" * n)
        self.pos += n

    def clean_until(self, residue):
        """at least 150 bases (every k <= 64 sees whole windows again), up to a position = residue (mod 64)"""
        self.bases(150)
        self.bases((residue - self.pos) % 64)

    def fasta(self):
        return np.frombuffer(("".join(self.text) + "\n").encode(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _genomes():
    s = _Stream("k1 windows")
    s.header()
    s.bases(3 * 64 + 5)
    for by_record in (False, True):
        for e in EDGES:
            s.clean_until((e - 1) % 64)      # the BREAK goes here, the first clean token behind it at e (mod 64)
            if by_record:
                s.header()
            else:
                s.ns(1)
            s.first_clean.append(s.pos)
            assert s.pos % 64 == e % 64
    s.clean_until(37)
    s.ns(70)
    s.first_clean.append(s.pos)
    assert s.pos < TILE          # all of it inside the first tile
    # across the tile edge: the BREAK is the last token of tile 0, the first clean token the first of tile 1
    s.bases(TILE - 1 - s.pos)
    s.ns(1)
    s.first_clean.append(s.pos)
    s.bases(NTOK - s.pos)
    assert s.pos == NTOK
    short = np.frombuffer(b">short\n" + "".join(random.Random("k1 short").choice("ACGT") for _ in range(50)).encode() + b"\n", dtype=np.uint8)
    return s.fasta(), short, tuple(s.first_clean), tuple(s.rec_starts)


def test_breaks_sit_at_the_word_edges(tmp_path):
    """the input is what the docstring says: record starts and stream length as the library's own record index gives them"""
    from dandd_amd.engine import fasta_index
    fa, short, first_clean, rec_starts = _genomes()
    path = tmp_path / "g0.fa"
    path.write_bytes(fa.tobytes())
    _, _, tok_start, ntok = fasta_index(str(path))
    assert ntok == NTOK and tuple(int(t) for t in tok_start) == rec_starts
    assert sorted({p % 64 for p in first_clean[:32]}) == sorted({e % 64 for e in EDGES})
    assert {p % 16 for p in first_clean[:32]} == {14, 15, 0, 1}
    path.write_bytes(short.tobytes())
    assert fasta_index(str(path))[3] == 51


@functools.lru_cache(maxsize=None)
def _want(orc, krange, p, canonical):
    fa, short = _genomes()[:2]
    return [orc.sketch_sweep(f, krange[0], krange[1], p, canonical) for f in (fa, short)]


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("p", [14, 17])
@pytest.mark.parametrize("krange", K_RANGES, ids=lambda r: f"k{r[0]}-{r[1]}")
def test_windows_at_every_word_edge(engine_factory, torch_cuda, orc, monkeypatch, krange, p, canonical):
    torch = torch_cuda
    if p >= 17:
        monkeypatch.setenv("DD_BUCKET_E0", "1")
        monkeypatch.setenv("DD_BUCKET_EMAX", "1")
    eng = engine_factory(p, canonical)
    fas = _genomes()[:2]
    kmin, kmax = krange
    bufs = []
    for fa in fas:
        t = torch.zeros(fa.size + 16, dtype=torch.uint8, device="cuda")
        t[:fa.size] = torch.from_numpy(fa.copy())
        bufs.append(t)
    slab = torch.empty((len(fas), kmax - kmin + 1, 1 << p), dtype=torch.uint8, device="cuda")
    eng.sketch_device([b.data_ptr() for b in bufs], [fa.size for fa in fas], kmin, kmax, slab.data_ptr())
    eng.synchronize()
    got = slab.cpu().numpy()
    for g, want in enumerate(_want(orc, krange, p, canonical)):
        bad = np.argwhere(got[g] != want)
        assert bad.size == 0, (f"genome {g}: {bad.shape[0]} registers differ, first at (k={kmin + bad[0][0]}, idx={bad[0][1]}): "
                               f"got {got[g][tuple(bad[0])]} want {want[tuple(bad[0])]}")
