"""dd_cross on the MI355X: the rectangle |a_s U b_j| of two register slabs.

The yardstick is the square that was there before: dd_pairwise_device on the rows of both slabs behind one another holds the
rectangle at [s][na + j].  Then the Gram form against the streaming kernel, the register range over both slabs against the
oracle, the three forms of the entry, the rounds, the argument rules and HipBackend.cross_cards."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (log2m, na, nb, K): the smallest shapes that reach the half-height form alone (na <= 32), the full form alone (na = 64), both in
# one call (33 = no half block, 65 and 130 = full blocks and a half one), one and several B blocks, padding rows on both sides,
# more than 64 k columns, several register ranges per row (log2m 18, 20)
SHAPES = [(12, 1, 1, 3), (12, 1, 65, 3), (14, 31, 64, 2), (14, 32, 63, 3), (14, 33, 129, 2), (14, 64, 64, 2), (14, 65, 257, 2),
          (13, 130, 70, 2), (14, 3, 5, 70), (18, 2, 65, 2), (20, 3, 64, 2)]

# trailing zeros of a random byte + 1: a geometric(1/2) value, cut at 9 -- what rng.geometric gives, at the cost of a table look-up
_GEO = np.array([min(9, (b & -b).bit_length()) if b else 9 for b in range(256)], dtype=np.uint8)


def _slab(rng, n, K, p):
    """A slab shaped as test_gpu_parity._random_slab shapes it: geometric registers with a per-row offset, capped at q + 1 =
    64 - p + 1, 5 % empty; with K >= 3 a constant column, an empty column and one that uses every value, with the corner bytes."""
    m, q = 1 << p, 64 - p
    slab = np.minimum(_GEO[rng.integers(0, 256, size=(n, K, m), dtype=np.uint8)] + rng.integers(0, 3, size=(n, K, 1), dtype=np.uint8), q + 1)
    slab = slab.astype(np.uint8)
    slab[rng.integers(0, 20, size=(n, K, m), dtype=np.uint8) == 0] = 0
    if K >= 3:
        slab[:, 0, :] = 7
        slab[:, 1, :] = 0
        slab[:, 2, :] = rng.integers(0, q + 2, size=(n, m), dtype=np.uint8)
        slab[0, 2, :5] = [0, q + 1, q + 1, 0, q]
    return slab


_CASES = {}


def _case(engine_factory, torch, shape):
    """The slabs of a shape, on the host and on the device, and the square of the rows of both -- made once per shape"""
    if shape not in _CASES:
        p, na, nb, K = shape
        rng = np.random.default_rng(((p * 1009 + na) * 1009 + nb) * 1009 + K)
        a, b = _slab(rng, na, K, p), _slab(rng, nb, K, p)
        both = torch.from_numpy(np.concatenate([a, b])).cuda()
        square = engine_factory(p, True).pairwise_device(both.data_ptr(), na + nb, K)
        da, db = both[:na], both[na:]
        _CASES[shape] = (a, b, da, db, square[:na, na:].copy(), both)
    return _CASES[shape][:5]


@pytest.mark.parametrize("shape", SHAPES)
def test_cross_equals_the_square_of_both_slabs(engine_factory, torch_cuda, monkeypatch, shape):
    """cross_device(A, B)[s, j, k] == pairwise_device(concat(A, B))[s, na + j, k] as doubles, for every entry; the same call
    with DD_CROSS_STREAM=1 gives the same table; last_k2_path names the kernel that ran (DD_K2_CROSS_GRAM 6 from log2m 12 on,
    DD_K2_CROSS_STREAM 5 when asked for)."""
    p, na, nb, K = shape
    eng = engine_factory(p, True)
    a, b, da, db, want = _case(engine_factory, torch_cuda, shape)
    monkeypatch.delenv("DD_CROSS_STREAM", raising=False)
    monkeypatch.delenv("DD_CROSS_HIST_MB", raising=False)
    gram = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_gram" and eng._lib.dd_last_k2_path(eng._ctx) == 6
    assert gram.shape == (na, nb, K)
    bad = np.argwhere(gram != want)
    assert bad.size == 0, f"{len(bad)} of {gram.size} entries differ from the square, first (s, j, k) = {bad[0]}: {gram[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_stream" and eng._lib.dd_last_k2_path(eng._ctx) == 5
    bad = np.argwhere(gram != stream)
    assert bad.size == 0, f"{len(bad)} of {gram.size} entries differ from the streaming kernel, first (s, j, k) = {bad[0]}"


def test_small_sketches_take_the_streaming_kernel(engine_factory, torch_cuda, orc, monkeypatch):
    monkeypatch.delenv("DD_CROSS_STREAM", raising=False)
    p, na, nb, K = 10, 3, 5, 3
    eng = engine_factory(p, True)
    rng = np.random.default_rng(10)
    a, b = _slab(rng, na, K, p), _slab(rng, nb, K, p)
    got = eng.cross(a, b)
    assert eng.last_k2_path() == "cross_stream"
    want = np.array([[[orc.card(np.maximum(a[s, k], b[j, k]), p) for k in range(K)] for j in range(nb)] for s in range(na)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", ["a_empty", "a_above_b", "b_above_a"])
def test_register_range_covers_both_slabs(engine_factory, orc, monkeypatch, case):
    """A column's thresholds run from the smallest to the largest register of BOTH slabs.  With A all zero, A's own range is
    empty and B's would be missed from A; with every A register above B's largest (or the reverse) the range of either slab
    alone leaves out the thresholds at which the other slab's rows change -- every entry against the oracle on the byte-max."""
    monkeypatch.delenv("DD_CROSS_STREAM", raising=False)
    p, na, nb, K = 12, 3, 5, 2
    m = 1 << p
    eng = engine_factory(p, True)
    rng = np.random.default_rng(77)
    a, b = _slab(rng, na, K, p), _slab(rng, nb, K, p)
    if case == "a_empty":
        a[:] = 0
    elif case == "a_above_b":
        a[:, 0, :] = rng.integers(20, 30, size=(na, m), dtype=np.uint8)
        b[:, 0, :] = rng.integers(2, 9, size=(nb, m), dtype=np.uint8)
    else:
        b[:, 0, :] = rng.integers(20, 30, size=(nb, m), dtype=np.uint8)
        a[:, 0, :] = rng.integers(2, 9, size=(na, m), dtype=np.uint8)
    got = eng.cross(a, b)
    assert eng.last_k2_path() == "cross_gram"
    want = np.array([[[orc.card(np.maximum(a[s, k], b[j, k]), p) for k in range(K)] for j in range(nb)] for s in range(na)])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {got.size} entries differ from the oracle, first (s, j, k) = {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def test_forms_rounds_and_repeats_give_the_same_bytes(engine_factory, torch_cuda, monkeypatch):
    """host / host == device / device == host A with device B, byte for byte; a budget of 1 MiB of histograms makes several
    rounds (130 rows of A: three 64-row blocks, 257 x 2 x 256 bytes x 64 rows = 8 MiB a block) and the same table; two calls
    give identical bytes."""
    monkeypatch.delenv("DD_CROSS_STREAM", raising=False)
    monkeypatch.delenv("DD_CROSS_HIST_MB", raising=False)
    shape = (14, 130, 257, 2)
    p, na, nb, K = shape
    eng = engine_factory(p, True)
    a, b, da, db, want = _case(engine_factory, torch_cuda, shape)
    dd = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert np.array_equal(dd, want)
    assert eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K).tobytes() == dd.tobytes()
    assert eng.cross(a, b).tobytes() == dd.tobytes()
    assert eng.cross_host_device(a, db.data_ptr(), nb).tobytes() == dd.tobytes()
    monkeypatch.setenv("DD_CROSS_HIST_MB", "1")
    assert eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K).tobytes() == dd.tobytes()
    assert eng.cross_host_device(a, db.data_ptr(), nb).tobytes() == dd.tobytes()
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    assert eng.cross(a, b).tobytes() == dd.tobytes()


def test_argument_rules_are_pairwise_s(engine_factory, torch_cuda):
    from dandd_amd.engine import EngineError
    eng = engine_factory(12, True)
    t = torch_cuda.zeros(4 << 12, dtype=torch_cuda.uint8, device="cuda")
    ptr = t.data_ptr()
    with pytest.raises(EngineError) as square:
        eng.pairwise_device(ptr, 0, 1)
    for args in ((ptr, 0, ptr, 2, 2), (ptr, 2, ptr, 0, 2), (ptr, 2, ptr, 2, 0), (0, 2, ptr, 2, 2), (ptr, 2, 0, 2, 2)):
        with pytest.raises(EngineError) as err:
            eng.cross_device(*args)
        assert err.value.code == -1 and str(err.value) == str(square.value), (args, str(err.value))
    with pytest.raises(EngineError) as err:
        eng.cross_host_device(np.zeros((1, 1, 1 << 12), dtype=np.uint8), 0, 1)
    assert err.value.code == -1


def test_backend_cross_cards(tmp_path, torch_cuda, orc, monkeypatch):
    """HipBackend.cross_cards on 3 samples x 5 leaves of 40 kbp at log2m 12 against the oracle's union + card; a sample that
    is leaf 2 has the leaf's own cards against itself; the slab in HBM is the same object before and after; the host form
    (DANDD_DEVICE_CACHE_MB=0) and the merged form agree with the oracle too."""
    from dandd_amd.host import backend as B
    monkeypatch.delenv("DD_CROSS_STREAM", raising=False)
    rng = np.random.default_rng(5)
    p, lo, hi = 12, 9, 12

    def fasta(name, n):
        path = os.path.join(str(tmp_path), name)
        with open(path, "wb") as f:
            f.write(b">g\n" + rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tobytes() + b"\n")
        return path
    leaves = [fasta(f"g{g}.fasta", 40000 + 1000 * g) for g in range(5)]
    samples = [fasta("s0.fasta", 40000), leaves[2], fasta("s2.fasta", 20000)]
    be = B.HipBackend(p, True)
    path_of = lambda i, k: os.path.join(str(tmp_path), f"s{i}.w.{k}.spacing.{p}.hll")
    be.leaf_many(leaves, lo, hi, path_of)
    paths = [[path_of(i, k) for k in range(lo, hi + 1)] for i in range(5)]
    order = [3, 0, 4, 1, 2]                                     # (not the slab's own order: the columns go back through perm)
    listed = [paths[i] for i in order]
    pair = be.pairwise_cards(listed)
    dev = be._dev
    assert dev is not None
    regs = be.sample_sketches(samples, lo, hi)
    assert regs.shape == (3, hi - lo + 1, 1 << p)
    got = be.cross_cards(regs, listed)
    assert be._dev is dev and be.engine.last_k2_path() == "cross_gram"
    slab = [[B.read_sketch_file(q)[0] for q in row] for row in listed]
    want = np.array([[[orc.card(np.maximum(regs[s, kk], slab[j][kk]), p) for kk in range(hi - lo + 1)] for j in range(5)] for s in range(3)])
    assert np.array_equal(got, want)
    at = order.index(2)
    assert np.array_equal(got[1, at], pair[at, at]) and np.array_equal(be.sample_cards(regs[1]), pair[at, at])
    merged = be.cross_cards(regs, listed, merged=True)
    assert be._dev is dev and merged.shape == (3, 1, hi - lo + 1)
    whole = [np.maximum.reduce([slab[j][kk] for j in range(5)]) for kk in range(hi - lo + 1)]
    assert np.array_equal(merged[:, 0], np.array([[orc.card(np.maximum(regs[s, kk], whole[kk]), p) for kk in range(hi - lo + 1)] for s in range(3)]))
    monkeypatch.setenv("DANDD_DEVICE_CACHE_MB", "0")
    be2 = B.HipBackend(p, True)
    assert np.array_equal(be2.cross_cards(regs, listed), want) and be2._dev is None
    be.close()
    be2.close()
