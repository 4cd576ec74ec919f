"""The Gram forms of dd_pairwise and dd_cross (dd_gram.hip) where their launchers cut the work into several launches, and three
value corners of the same kernels.

A launch of gram_kernel / cross_kernel covers as many units (blocks of 64 or 128 rows against one another) as fit the budget of
partial counts, 1 GiB by default: at the shapes a test can afford that is every unit, sp_base is 0 and the split never runs.
DD_GRAM_PART_MB makes the budget small, dd_last_k2_launches counts the launches that ran.  Every split call is compared with
the streaming kernels of dd_union.hip (DD_PAIRWISE_STREAM=1 / DD_CROSS_STREAM=1: another implementation of the same histograms)
entry by entry, with the same call at the default budget byte for byte, and with the oracle's estimator on the byte-max at seeded
entries that include the LAST unit of each form -- a kernel that lost sp_base would leave the units after the first of every
launch unwritten (0.0 in the square, whose histograms the caller zeroes) and write the first unit's rows from another pair."""
import numpy as np
import pytest

from test_gpu_cross import _GEO, _slab

pytestmark = pytest.mark.gpu

KNOBS = ("DD_PAIRWISE_STREAM", "DD_CROSS_STREAM", "DD_CROSS_HIST_MB", "DD_GRAM_PART_MB")


def _clear(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


# ---- the launchers' arithmetic, restated -------------------------------------------------------------------------------------
# dd_gram.hip: gram_len, gram_slots, gram_part_budget, gram_scratch_bytes (the square's `fit`), cross_scratch_bytes (the
# rectangle's), and the loops of launch_pairwise_gram and launch_cross_gram over the units of each form; dd_k2_api.hip: the rounds
# of cross() over a's 64-row blocks under DD_CROSS_HIST_MB.
def _gram_len(nsp, K, p):
    m = 1 << p
    ln = min(m, 1 << 16)
    while ln > 1024 and nsp * K * (m // ln) < 512:
        ln >>= 1
    return ln


def _fit(per_sp, total, part_mb):
    budget = (part_mb if part_mb and part_mb > 0 else 1024) << 20
    return max(1, min(total, budget // per_sp))


def _ceil(a, b):
    return -(-a // b)


def _square_plan(p, n, K, part_mb=None):
    """-> (fit, launches of the diagonal form, launches of kOff)"""
    ns = (n + 63) // 64
    d2 = n > 64
    RR = (1 << p) // _gram_len(4 * ((ns + 1) // 2) if d2 else ns, K, p)
    per_sp = K * RR * (64 - p + 1) * (10 if d2 else 4) * 1024 * 4
    fit = _fit(per_sp, ns * (ns + 1) // 2, part_mb)
    diag = (ns + 1) // 2 if d2 else ns
    off = ns * (ns - 1) // 2 - (ns // 2 if d2 else 0)
    return fit, _ceil(diag, fit), _ceil(off, fit)


def _cross_plan(p, na, nb, K, part_mb=None, hist_mb=None):
    """-> one (fit, launches of kCross, launches of kCrossHalf) per round of the call"""
    budget = (hist_mb if hist_mb and hist_mb > 0 else 1024) << 20
    per_block = 64 * nb * K * 64 * 4
    rows = 64 * min(max(budget // per_block, 1), (na + 63) // 64)
    plan = []
    for s0 in range(0, na, rows):
        cnt = min(rows, na - s0)
        nsa, nsb = (cnt + 63) // 64, (nb + 63) // 64
        RR = (1 << p) // _gram_len(nsa * nsb, K, p)
        per_sp = K * RR * (64 - p + 1) * 4 * 1024 * 4
        fit = _fit(per_sp, nsa * nsb, part_mb)
        nhalf = 1 if cnt - 64 * (nsa - 1) <= 32 else 0
        plan.append((fit, _ceil((nsa - nhalf) * nsb, fit), _ceil(nhalf * nsb, fit)))
    return plan


def _same_estimate(got, want):
    return got == want or (np.isinf(want) and np.isinf(got))


def _no_difference(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {got.size} entries differ from {what}, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


_SLABS = {}


def _slabs(torch, key, make):
    """host and device copies of a case's slabs, made once"""
    if key not in _SLABS:
        host = make()
        _SLABS[key] = (host, [torch.from_numpy(x).cuda() for x in host])
    return _SLABS[key]


# ---- 1. the square ----------------------------------------------------------------------------------------------------------
# (log2m, n, K), DD_GRAM_PART_MB, fit, launches: 130 = two kDiag2 units and two kOff units; 257 = the odd 64-row block and every
# `paired` skip of gram_pair<kOff> at a non-zero base; 64 MiB = a last launch with fewer units than fit; 192 x 3 = the corners
# columns; 64 rows = one unit, whatever the budget ("at least one")
SQUARE = [((12, 130, 2), 1, 1, 4), ((12, 257, 2), 1, 1, 11), ((12, 257, 2), 64, 3, 4), ((14, 192, 3), 1, 1, 4), ((12, 64, 3), 1, None, 1)]


def _square_entries(rng, n, K):
    """(i, j, k) for the oracle: the last unit of the diagonal form, the last unit of kOff, the first unit, and seeded ones"""
    ns = (n + 63) // 64
    picks = [(0, 0, 0), (n - 1, n - 1, K - 1)]
    if ns > 1:
        picks.append((128 * ((ns - 1) // 2), n - 1, 0))           # first row of the last kDiag2 unit against the last row of all
        P = ns - 2                                                 # the last unit of kOff is (P, ns - 1), P the largest block ...
        if P % 2 == 0:
            P -= 1                                                 # ... that is not paired with ns - 1 inside a kDiag2 unit
        if P >= 0:
            picks += [(64 * P + 5, n - 1, K - 1), (64 * P + 63, 64 * (ns - 1), 0)]
    while len(picks) < 10:
        i, j = sorted((int(rng.integers(n)), int(rng.integers(n))))
        picks.append((i, j, int(rng.integers(K))))
    return picks


@pytest.mark.parametrize("shape,part_mb,fit,launches", SQUARE)
def test_square_split_equals_streaming_unsplit_and_oracle(engine_factory, torch_cuda, orc, monkeypatch, shape, part_mb, fit, launches):
    _clear(monkeypatch)
    p, n, K = shape
    eng = engine_factory(p, True)
    rng = np.random.default_rng((p * 1009 + n) * 1009 + K)
    (slab,), (dev,) = _slabs(torch_cuda, ("square",) + shape, lambda: [_slab(rng, n, K, p)])
    whole = eng.pairwise_device(dev.data_ptr(), n, K)
    assert eng.last_k2_path() == "pairwise_gram" and eng.last_k2_launches() == sum(_square_plan(p, n, K)[1:])
    monkeypatch.setenv("DD_GRAM_PART_MB", str(part_mb))
    got_fit, diag, off = _square_plan(p, n, K, part_mb)
    assert diag + off == launches and (fit is None or got_fit == fit), (got_fit, diag, off)
    split = eng.pairwise_device(dev.data_ptr(), n, K)
    assert eng.last_k2_path() == "pairwise_gram"
    print(f"square {shape} DD_GRAM_PART_MB={part_mb}: fit {got_fit}, launches {eng.last_k2_launches()} (derived {diag} + {off})")
    assert eng.last_k2_launches() == launches
    assert launches > 1 or n <= 64
    monkeypatch.setenv("DD_PAIRWISE_STREAM", "1")
    stream = eng.pairwise_device(dev.data_ptr(), n, K)
    assert eng.last_k2_path() == "pairwise_stream" and eng.last_k2_launches() == 0
    _no_difference(split, stream, "the streaming kernel")
    assert split.tobytes() == whole.tobytes()
    assert np.array_equal(split, split.transpose(1, 0, 2))
    for i, j, k in _square_entries(rng, n, K):
        want = orc.card(np.maximum(slab[i, k], slab[j, k]), p)
        assert _same_estimate(split[i, j, k], want), (i, j, k, split[i, j, k], want)


# ---- 2. the rectangle -------------------------------------------------------------------------------------------------------
# (log2m, na, nb, K), DD_GRAM_PART_MB, fit, launches: the half-height form alone, full and half, a fit of 3 over 4 full units and
# 2 half ones, the full form alone with the corners columns
CROSS = [((12, 3, 130, 2), 1, 1, 3), ((12, 65, 130, 2), 1, 1, 6), ((13, 130, 70, 2), 40, 3, 3), ((14, 64, 129, 3), 1, 1, 3)]


def _cross_entries(rng, na, nb, K):
    """(s, j, k) for the oracle: the last unit of the full form, the last unit of the half form, the first unit, seeded ones"""
    nsa, nsb = (na + 63) // 64, (nb + 63) // 64
    nhalf = 1 if na - 64 * (nsa - 1) <= 32 else 0
    picks = [(0, 0, 0), (na - 1, nb - 1, K - 1)]
    if nsa - nhalf:
        top = min(na, 64 * (nsa - nhalf)) - 1                      # last row of the last full block of a
        picks += [(top, nb - 1, 0), (64 * (nsa - nhalf - 1), 64 * (nsb - 1), K - 1)]
    if nhalf:
        picks += [(64 * (nsa - 1), 64 * (nsb - 1), 0), (na - 1, 64 * (nsb - 1), K - 1)]
    while len(picks) < 10:
        picks.append((int(rng.integers(na)), int(rng.integers(nb)), int(rng.integers(K))))
    return picks


def _cross_slabs(torch, shape):
    p, na, nb, K = shape
    rng = np.random.default_rng(((p * 1009 + na) * 1009 + nb) * 1009 + K + 1)
    return rng, _slabs(torch, ("cross",) + shape, lambda: [_slab(rng, na, K, p), _slab(rng, nb, K, p)])


@pytest.mark.parametrize("shape,part_mb,fit,launches", CROSS)
def test_cross_split_equals_streaming_unsplit_and_oracle(engine_factory, torch_cuda, orc, monkeypatch, shape, part_mb, fit, launches):
    _clear(monkeypatch)
    p, na, nb, K = shape
    eng = engine_factory(p, True)
    rng, ((a, b), (da, db)) = _cross_slabs(torch_cuda, shape)
    whole = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_gram" and eng.last_k2_launches() == sum(f + h for _, f, h in _cross_plan(p, na, nb, K))
    monkeypatch.setenv("DD_GRAM_PART_MB", str(part_mb))
    ((got_fit, full, half),) = _cross_plan(p, na, nb, K, part_mb)
    assert got_fit == fit and full + half == launches, (got_fit, full, half)
    split = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_gram"
    print(f"cross {shape} DD_GRAM_PART_MB={part_mb}: fit {got_fit}, launches {eng.last_k2_launches()} (derived {full} + {half})")
    assert eng.last_k2_launches() == launches and launches > 1
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_stream" and eng.last_k2_launches() == 0
    _no_difference(split, stream, "the streaming kernel")
    assert split.tobytes() == whole.tobytes()
    for s, j, k in _cross_entries(rng, na, nb, K):
        want = orc.card(np.maximum(a[s, k], b[j, k]), p)
        assert _same_estimate(split[s, j, k], want), (s, j, k, split[s, j, k], want)


def test_cross_rounds_and_split_together(engine_factory, torch_cuda, orc, monkeypatch):
    """130 x 130 at log2m 12 with DD_CROSS_HIST_MB=1 (a round per 64-row block of a: 64 + 64 + 2 rows) and DD_GRAM_PART_MB=1
    (fit 1): every round's a_round offset meets sp_base 1 and 2 -- three full launches in each of the first two rounds, three half
    ones in the last.  The bytes are the default call's, from slabs in HBM and with a from host memory."""
    _clear(monkeypatch)
    shape = (12, 130, 130, 2)
    p, na, nb, K = shape
    eng = engine_factory(p, True)
    rng, ((a, b), (da, db)) = _cross_slabs(torch_cuda, shape)
    whole = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_launches() == 2                                     # (six full units in one launch, three half ones in another)
    monkeypatch.setenv("DD_CROSS_HIST_MB", "1")
    monkeypatch.setenv("DD_GRAM_PART_MB", "1")
    plan = _cross_plan(p, na, nb, K, 1, 1)
    assert plan == [(1, 3, 0), (1, 3, 0), (1, 0, 3)]
    split = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    print(f"cross {shape} rounds and split: launches {eng.last_k2_launches()} (derived {plan})")
    assert eng.last_k2_path() == "cross_gram" and eng.last_k2_launches() == 9
    assert split.tobytes() == whole.tobytes()
    mixed = eng.cross_host_device(a, db.data_ptr(), nb)
    assert eng.last_k2_launches() == 9 and mixed.tobytes() == whole.tobytes()
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_launches() == 0
    _no_difference(split, stream, "the streaming kernel")
    for s, j, k in _cross_entries(rng, na, nb, K):
        want = orc.card(np.maximum(a[s, k], b[j, k]), p)
        assert _same_estimate(split[s, j, k], want), (s, j, k, split[s, j, k], want)


# ---- 3. value corners -------------------------------------------------------------------------------------------------------
def _headroom_slab(rng, n, K, p, first):
    """column 0: 7 in every register (8 in register 0 of row 0 of the slab that is `first`) -- one threshold, 7, at which every
    register of every pair counts but register 0 of a pair with that row; column 1: geometric"""
    m = 1 << p
    slab = np.empty((n, K, m), dtype=np.uint8)
    slab[:, 0] = 7
    if first:
        slab[0, 0, 0] = 8
    for kk in range(1, K):
        slab[:, kk] = np.minimum(_GEO[rng.integers(0, 256, size=(n, m), dtype=np.uint8)], 64 - p + 1)
    return slab


def test_square_accumulator_headroom(engine_factory, torch_cuda, orc, monkeypatch):
    """(20, 3, 2): every register at or under the one threshold of column 0.  At this shape gram_len shares the row out over
    enough workgroups to fill the chip -- 4096 registers a wave, 2^26 in the accumulator; the cases of
    test_accumulator_at_two_to_the_thirty below keep 2^16 registers a wave."""
    _clear(monkeypatch)
    p, n, K = 20, 3, 2
    eng = engine_factory(p, True)
    rng = np.random.default_rng(2030)
    (slab,), (dev,) = _slabs(torch_cuda, ("headroom", p, n, K), lambda: [_headroom_slab(rng, n, K, p, True)])
    gram = eng.pairwise_device(dev.data_ptr(), n, K)
    assert eng.last_k2_path() == "pairwise_gram"
    monkeypatch.setenv("DD_PAIRWISE_STREAM", "1")
    stream = eng.pairwise_device(dev.data_ptr(), n, K)
    assert eng.last_k2_path() == "pairwise_stream"
    _no_difference(gram, stream, "the streaming kernel")
    for i, j in ((0, 0), (0, 1), (1, 2)):
        want = orc.card(np.maximum(slab[i, 0], slab[j, 0]), p)
        assert gram[i, j, 0] == want and gram[j, i, 0] == want, (i, j, gram[i, j, 0], want)


@pytest.mark.parametrize("shape", [(20, 2, 3, 2), (20, 64, 2, 1)])
def test_cross_accumulator_headroom(engine_factory, torch_cuda, orc, monkeypatch, shape):
    """(20, 2, 3, 2): the half-height form; (20, 64, 2, 1): the full form.  Column 0 against the oracle at (0, 0), (0, 1) and
    (1, 2) -- (1, 1) where b has two rows."""
    _clear(monkeypatch)
    p, na, nb, K = shape
    eng = engine_factory(p, True)
    rng = np.random.default_rng(2031 + na)
    (a, b), (da, db) = _slabs(torch_cuda, ("headroom",) + shape,
                              lambda: [_headroom_slab(rng, na, K, p, True), _headroom_slab(rng, nb, K, p, False)])
    gram = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_gram"
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = eng.cross_device(da.data_ptr(), na, db.data_ptr(), nb, K)
    assert eng.last_k2_path() == "cross_stream"
    _no_difference(gram, stream, "the streaming kernel")
    for s, j in ((0, 0), (0, 1), (1, min(2, nb - 1))):
        want = orc.card(np.maximum(a[s, 0], b[j, 0]), p)
        assert gram[s, j, 0] == want, (s, j, gram[s, j, 0], want)


# 2^16 registers a wave need K x units x 16 >= 512 workgroups (gram_len): 32 columns at log2m 20.  Every column is constant but
# for ONE register, so the slabs are written on the device; the oracle gets the two rows there are.
@pytest.mark.parametrize("form,na,nb", [("square", 3, 0), ("half", 2, 3), ("full", 33, 1)])
def test_accumulator_at_two_to_the_thirty(engine_factory, torch_cuda, orc, monkeypatch, form, na, nb):
    """Column kk holds c = 1 + kk % 20 in every register, c + 1 in register 0 of row 0: one threshold, c, and every register
    range but the first of a pair with row 0 counts all 65 536 of its registers -- 2^16 hits x 2^14 = 2^30 in the int32
    accumulator.  Every entry against the streaming kernel, and against the oracle (a table of two values per column)."""
    _clear(monkeypatch)
    torch = torch_cuda
    p, K = 20, 32
    m = 1 << p
    eng = engine_factory(p, True)
    assert _gram_len(1, K, p) == 1 << 16
    consts = (1 + torch.arange(K, dtype=torch.uint8, device="cuda") % 20).reshape(1, K, 1)
    a = consts.expand(na, K, m).contiguous()
    a[0, :, 0] += 1
    if form == "square":
        call = lambda: eng.pairwise_device(a.data_ptr(), na, K)
    else:
        b = consts.expand(nb, K, m).contiguous()
        call = lambda: eng.cross_device(a.data_ptr(), na, b.data_ptr(), nb, K)
    gram = call()
    assert eng.last_k2_path() == ("pairwise_gram" if form == "square" else "cross_gram")
    monkeypatch.setenv("DD_PAIRWISE_STREAM", "1")
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = call()
    assert eng.last_k2_path() == ("pairwise_stream" if form == "square" else "cross_stream")
    _no_difference(gram, stream, "the streaming kernel")
    want = np.empty_like(gram)
    for kk in range(K):
        row = np.full(m, 1 + kk % 20, dtype=np.uint8)
        plain = orc.card(row, p)
        row[0] += 1
        want[..., kk] = plain
        want[0, ..., kk] = orc.card(row, p)
        if form == "square":
            want[:, 0, kk] = want[0, 0, kk]
    _no_difference(gram, want, "the oracle")
    del a


@pytest.mark.parametrize("va,vb,na,nb", [(0, 0, 3, 5), (5, 5, 3, 5), (0, 5, 3, 5), (0, 0, 64, 70), (5, 5, 64, 70), (0, 5, 70, 3)])
def test_cross_of_constant_slabs(engine_factory, torch_cuda, orc, monkeypatch, va, vb, na, nb):
    """Every column constant (both slabs zero -- the empty sample against an empty collection --, both 5): no workgroup of
    cross_kernel has work, cross_finish_kernel alone writes the histograms.  A zero against B = 5 has five thresholds."""
    _clear(monkeypatch)
    p, K = 12, 2
    eng = engine_factory(p, True)
    a, b = np.full((na, K, 1 << p), va, dtype=np.uint8), np.full((nb, K, 1 << p), vb, dtype=np.uint8)
    gram = eng.cross(a, b)
    assert eng.last_k2_path() == "cross_gram"
    monkeypatch.setenv("DD_CROSS_STREAM", "1")
    stream = eng.cross(a, b)
    assert eng.last_k2_path() == "cross_stream"
    want = np.full((na, nb, K), orc.card(np.maximum(a[0, 0], b[0, 0]), p))
    assert va or vb or not want.any()                                      # (both empty: 0.0 everywhere)
    assert np.array_equal(gram, want) and np.array_equal(stream, want)


@pytest.mark.parametrize("value,n", [(0, 3), (5, 70)])
def test_square_of_a_constant_slab(engine_factory, torch_cuda, orc, monkeypatch, value, n):
    _clear(monkeypatch)
    p, K = 12, 2
    eng = engine_factory(p, True)
    slab = np.full((n, K, 1 << p), value, dtype=np.uint8)
    gram = eng.pairwise(slab)
    assert eng.last_k2_path() == "pairwise_gram"
    monkeypatch.setenv("DD_PAIRWISE_STREAM", "1")
    stream = eng.pairwise(slab)
    assert eng.last_k2_path() == "pairwise_stream"
    want = np.full((n, n, K), orc.card(slab[0, 0], p))
    assert value or not want.any()
    assert np.array_equal(gram, want) and np.array_equal(stream, want)


@pytest.mark.parametrize("p", [4, 6, 9, 11])
def test_streaming_rectangle_at_small_log2m(engine_factory, torch_cuda, orc, monkeypatch, p):
    """cross_stream_kernel is the only form under log2m 12; its workgroup (threads_for) and its tiles change shape from log2m 4
    to 9.  3 x 5 rows, the corners columns, registers up to 64 - log2m + 1: every entry against the oracle on the byte-max."""
    _clear(monkeypatch)
    na, nb, K = 3, 5, 3
    eng = engine_factory(p, True)
    rng = np.random.default_rng(400 + p)
    a, b = _slab(rng, na, K, p), _slab(rng, nb, K, p)
    assert max(a.max(), b.max()) == 64 - p + 1
    got = eng.cross(a, b)
    assert eng.last_k2_path() == "cross_stream" and eng.last_k2_launches() == 0
    want = np.array([[[orc.card(np.maximum(a[s, k], b[j, k]), p) for k in range(K)] for j in range(nb)] for s in range(na)])
    bad = np.argwhere(~((got == want) | (np.isinf(got) & np.isinf(want))))
    assert bad.size == 0, f"{len(bad)} of {got.size} entries differ from the oracle, first (s, j, k) = {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
