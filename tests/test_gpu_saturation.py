"""K1 saturation exit (dd_kernels.h, dd_sweep.hip: sweep_kernel, universe_kernel): a row of k = 10..14 that equals sketch(U_k),
the row every (canonical) k-mer hashed once gives, is final; sweep_kernel flags it at its merge and jobs that start later
leave it out.  Registers must stay bit for bit the oracle's: with the exit firing mid-stream, with it one register short
of firing, and with DD_NO_SATURATE=1.

A call's first 512 jobs (two workgroups per CU) start together, before any flag can be up, so the cases in which the exit must
be SEEN to act, or not to act, sketch the same device buffers several times in one call: the jobs of the last tiles then start
after the jobs of the first have merged."""
import numpy as np
import pytest

import pyref
from test_gpu_parity import _sweep_check

pytestmark = pytest.mark.gpu

K = 10


def _revcomp(x, k):
    x = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(x)
    for j in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((x >> np.uint64(2 * j)) & np.uint64(3)))
    return r


def _wang64(x):
    """Thomas Wang's mix on a uint64 array (wrap-around arithmetic); pinned to tests/pyref.py where it is used"""
    with np.errstate(over="ignore"):
        x = (~x) + (x << np.uint64(21))
        x ^= x >> np.uint64(24)
        x = x + (x << np.uint64(3)) + (x << np.uint64(8))
        x ^= x >> np.uint64(14)
        x = x + (x << np.uint64(2)) + (x << np.uint64(4))
        x ^= x >> np.uint64(28)
        x = x + (x << np.uint64(31))
    return x


_UNIVERSE = {}


def _universe(canonical):
    """the values of U_10 that are hashed: every 10-mer, or the smaller of each (10-mer, reverse complement)"""
    if canonical not in _UNIVERSE:
        x = np.arange(1 << (2 * K), dtype=np.uint64)
        _UNIVERSE[canonical] = x[x <= _revcomp(x, K)] if canonical else x
        assert _UNIVERSE[canonical].size == ((1 << 19) + (1 << 9) if canonical else 1 << 20)
    return _UNIVERSE[canonical]


def _records(xs):
    """one FASTA record per k-mer: '>', newline, its ten bases, newline"""
    out = np.empty((xs.size, K + 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, -1] = ord(">"), 10, 10
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(K):
        out[:, 2 + j] = acgt[((xs >> np.uint64(2 * (K - 1 - j))) & np.uint64(3)).astype(np.intp)]
    return out.reshape(-1)


def _lone_maximum(canonical, p):
    """a k-mer x of U_10 that alone holds the maximum of its register at log2m p (several k-mers share every register: 8 at the
    least).  Shortlisted with numpy, then established with the Python reference over ALL the k-mers of that register."""
    xs = _universe(canonical)
    h = _wang64(xs.copy())
    idx = (h >> np.uint64(64 - p)).astype(np.int64)
    for r in range(1 << p):
        members = [int(v) for v in xs[idx == r]]
        rhos = []
        for v in members:
            i, rho = pyref.idx_rho(pyref.wang64(v), p)
            assert i == r
            rhos.append(rho)
        top = max(rhos)
        if len(members) >= 2 and rhos.count(top) == 1:
            return members[rhos.index(top)], r, top
    raise AssertionError("no register with a lone maximum")


def _text_without(x, n, seed):
    """n random bases in which neither x nor its reverse complement occurs, as one record"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, n, dtype=np.uint8)
    banned = (np.uint64(x), _revcomp(np.uint64(x), K))
    while True:
        w = np.zeros(n - K + 1, dtype=np.uint64)
        for j in range(K):
            w = (w << np.uint64(2)) | codes[j:n - K + 1 + j].astype(np.uint64)
        hits = np.flatnonzero((w == banned[0]) | (w == banned[1]))
        if hits.size == 0:
            break
        codes[hits] = (codes[hits] + rng.integers(1, 4, hits.size, dtype=np.uint8)) & 3
    return np.concatenate([np.frombuffer(b">filler\n", dtype=np.uint8), np.frombuffer(b"ACGT", dtype=np.uint8)[codes], np.frombuffer(b"\n", dtype=np.uint8)])


def _sketch_batch(torch, eng, bufs, sizes, order, kmin, kmax):
    """one dd_sketch_device call over bufs[i] for i in order -> [len(order)][K][m]"""
    regs = torch.empty((len(order), kmax - kmin + 1, eng.m), dtype=torch.uint8, device="cuda")
    eng.sketch_device([bufs[i].data_ptr() for i in order], [sizes[i] for i in order], kmin, kmax, regs.data_ptr())
    eng.synchronize()
    return regs.cpu().numpy()


# ---- saturating mid-stream: the exit fires and changes nothing ---------------------------------------------------------------
_SYNTH = {}


def _synth(orc, n):
    if n not in _SYNTH:
        _SYNTH[n] = orc.synth_fasta(7, 0, n, 3)
    return _SYNTH[n]


def _saturates_within(orc, fa, k, p, canonical, eighths=6):
    """is the sketch of the first 3/4 (or eighths / 8) of the bytes already the sketch of the whole, for k?"""
    return np.array_equal(orc.sketch(fa[:fa.size * eighths // 8], k, p, canonical), orc.sketch(fa, k, p, canonical))


MID_STREAM = {
    # name: (bases, log2m, canonical, kmin, kmax, the k whose row saturates, does it within 3/4 of the bytes)
    # (the forward strand's k = 10 at log2m 10 does after 85 %: within 7/8, asserted too)
    "8M_k9_13_across_the_bitmap_boundary": (8_000_000, 10, True, 9, 13, 10, True),
    "8M_k10_alone": (8_000_000, 10, True, 10, 10, 10, True),
    "8M_k10_log2m14": (8_000_000, 14, True, 10, 10, 10, True),
    "24M_k10_12_log2m10": (24_000_000, 10, True, 10, 12, 11, True),
    "24M_k10_12_log2m14": (24_000_000, 14, True, 10, 12, 10, True),
    "8M_forward_strand_log2m10": (8_000_000, 10, False, 10, 12, 10, False),
    "8M_forward_strand_log2m14_does_not_saturate": (8_000_000, 14, False, 10, 12, 10, False),
}


@pytest.mark.parametrize("name", sorted(MID_STREAM))
def test_rows_that_saturate_mid_stream_match_the_oracle(engine_factory, orc, monkeypatch, name):
    n, p, canonical, kmin, kmax, ksat, saturates = MID_STREAM[name]
    fa = _synth(orc, n)
    assert _saturates_within(orc, fa, ksat, p, canonical) == saturates
    if name == "8M_forward_strand_log2m10":
        assert _saturates_within(orc, fa, ksat, p, canonical, eighths=7)
    monkeypatch.delenv("DD_NO_SATURATE", raising=False)
    monkeypatch.setenv("DD_SATURATE_ANY_SIZE", "1")   # (8 Mbp is under the gate of the forward strand's k = 10, 8 x 4^10 bytes)
    _sweep_check(engine_factory(p, canonical), orc, fa, kmin, kmax, canonical)


def test_late_jobs_of_a_saturated_row_leave_it_out_and_nothing_changes(engine_factory, torch_cuda, orc, monkeypatch):
    """The 8 Mbp input eight times in one call, k 10..12 at log2m 10: about a thousand one-tile jobs, of which those of the last third of the
    tiles start when k = 10 (after 49 % of the stream) has long been flagged.  And the same call under DD_NO_SATURATE=1."""
    torch = torch_cuda
    eng = engine_factory(10, True)
    fa = _synth(orc, 8_000_000)
    assert _saturates_within(orc, fa, 10, 10, True)
    want = orc.sketch_sweep(fa, 10, 12, 10, True)
    buf = torch.from_numpy(fa.copy()).cuda()
    monkeypatch.delenv("DD_SATURATE_ANY_SIZE", raising=False)
    for off in (False, True):
        if off:
            monkeypatch.setenv("DD_NO_SATURATE", "1")
        else:
            monkeypatch.delenv("DD_NO_SATURATE", raising=False)
        got = _sketch_batch(torch, eng, [buf], [fa.size], [0] * 8, 10, 12)
        for g in range(8):
            assert np.array_equal(got[g], want), f"genome {g}, DD_NO_SATURATE {'set' if off else 'unset'}"


# ---- the exit must not fire early -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("p", [14, 16])
def test_exit_does_not_fire_one_register_short(engine_factory, torch_cuda, orc, monkeypatch, p, canonical):
    """U_10 one record per k-mer WITHOUT x, the lone holder of its register's maximum; 2 Mbp of text with no x in it; x
    as the last record.  Until that record the row is one register short of sketch(U_10): an exit on "nearly equal", or on a
    stale word, loses exactly that register.  Beside it the same input with x in its place in the universe: there the row
    is final right behind the universe, and the exit may fire.  Four of each in one call (1080 jobs), k 10..11: groups of
    two at log2m 14, where the flagged k = 10 is dropped from the front of the group, single slots at log2m 16, where the job
    returns."""
    torch = torch_cuda
    eng = engine_factory(p, canonical)
    xs = _universe(canonical)
    x, reg, rho = _lone_maximum(canonical, p)
    filler = _text_without(x, 2_000_000, 1234 + p)
    last = _records(np.array([x], dtype=np.uint64))
    short = np.concatenate([_records(xs[xs != np.uint64(x)]), filler, last])
    whole = np.concatenate([_records(xs), filler, last])
    assert short.size + K + 3 == whole.size
    fas = [short, whole]
    want = [orc.sketch_sweep(f, 10, 11, p, canonical) for f in fas]
    # the preconditions, with the oracle: without its last record the short input lacks exactly register `reg`, the whole one nothing
    universe_row = orc.sketch(_records(xs), K, p, canonical)
    before = orc.sketch(short[:short.size - last.size], K, p, canonical)
    assert np.flatnonzero(before != universe_row).tolist() == [reg] and universe_row[reg] == rho and before[reg] < rho
    assert np.array_equal(want[0][0], universe_row) and np.array_equal(want[1][0], universe_row)
    monkeypatch.delenv("DD_NO_SATURATE", raising=False)
    monkeypatch.setenv("DD_SATURATE_ANY_SIZE", "1")
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    order = [0, 1] * 4
    got = _sketch_batch(torch, eng, bufs, [f.size for f in fas], order, 10, 11)
    for g, i in enumerate(order):
        bad = np.argwhere(got[g] != want[i])
        assert bad.size == 0, f"genome {g} ({'short' if i == 0 else 'whole'}): {bad.shape[0]} registers differ, first (k={10 + bad[0][0]}, idx={bad[0][1]}), x's register {reg}"


# ---- the builder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False])
def test_universe_input_and_a_strict_subset_of_it(engine_factory, torch_cuda, orc, monkeypatch, canonical):
    """The full universe and nothing else: its row IS sketch(U_10), whatever the builder made of its own.  Beside it, in the
    same call, every second k-mer: a row that differs and must not be taken for final."""
    torch = torch_cuda
    p = 12
    eng = engine_factory(p, canonical)
    xs = _universe(canonical)
    fas = [_records(xs), _records(xs[::2])]
    want = [orc.sketch(f, K, p, canonical) for f in fas]
    assert not np.array_equal(want[0], want[1])
    monkeypatch.delenv("DD_NO_SATURATE", raising=False)
    monkeypatch.setenv("DD_SATURATE_ANY_SIZE", "1")
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    order = [0, 1] * 3
    got = _sketch_batch(torch, eng, bufs, [f.size for f in fas], order, K, K)
    for g, i in enumerate(order):
        assert np.array_equal(got[g][0], want[i]), f"genome {g}"
