"""The C ABI's entries on register slabs (dd_k2_api.hip), each in its two forms -- the slab in host memory, the slab in HBM:
the two forms return the same doubles on the default and on a caller-owned stream, both refuse the same arguments with the
same words before anything is launched, and a call records the same number of DD_KERNEL_UNION spans in either form.

The smallest slab with more than one leaf, more than one column and an ordering that is not the identity: log2m 10, n = 3,
K = 2, registers drawn as test_gpu_parity._random_slab draws them, the second column empty in every leaf."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, N, K, KMIN = 10, 3, 2, 7
M = 1 << P
ORDS = [[0, 1, 2], [2, 0, 1]]
GROUPS = [0, -1, 1]
EINVAL = -1


@pytest.fixture(scope="module")
def slab():
    rng = np.random.default_rng(0x51AB)
    q = 64 - P
    s = np.minimum(rng.geometric(0.5, size=(N, K, M)) + rng.integers(0, 3, size=(N, K, 1)), q + 1).astype(np.uint8)
    s[rng.random((N, K, M)) < 0.05] = 0
    s[:, 1, :] = 0
    s.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def dev(slab, torch_cuda):
    """the slab in HBM and behind it leaf 2 again, a base row for extend_device, and a row for union_device to write"""
    t = torch_cuda.from_numpy(np.concatenate([slab, slab[2:], slab[:1]])).cuda()
    torch_cuda.cuda.synchronize()
    return t


@pytest.fixture(params=["default stream", "own stream"])
def eng(request, engine_factory, torch_cuda):
    e = engine_factory(P, True)
    if request.param == "own stream":
        stream = torch_cuda.cuda.Stream()
        e.set_stream(stream.cuda_stream)
    yield e
    e.set_stream(0)


def _card(orc, slab, rows, kk=0):
    return orc.card(np.maximum.reduce([slab[g, kk] for g in rows]), P)


# entry -> (the host form, the device form, (index, leaves): that cell of the result is the card of the union of those leaves at k column 0)
SCHEDULES = {
    "card_batch": (lambda e, s: e.card_batch(s), lambda e, d: e.card_batch_device(d, N * K), ((1 * K,), [1])),
    "progressive": (lambda e, s: e.progressive(s, ORDS), lambda e, d: e.progressive_device(d, N, K, ORDS), ((1, 1, 0), [2, 0])),
    "pairwise": (lambda e, s: e.pairwise(s), lambda e, d: e.pairwise_device(d, N, K), ((2, 0, 0), [0, 2])),
    "leave_out": (lambda e, s: e.leave_out(s, GROUPS), lambda e, d: e.leave_out_device(d, N, K, GROUPS), ((0, 0), [1, 2])),
    "subsets": (lambda e, s: e.subsets(s), lambda e, d: e.subsets_device(d, N, K), ((0b101, 0), [0, 2])),
    "extend, a base": (lambda e, s: e.extend(s[2], s), lambda e, d: e.extend_device(d + N * K * M, d, N, K), ((0, 0), [2, 0])),
    "extend, no base": (lambda e, s: e.extend(None, s), lambda e, d: e.extend_device(0, d, N, K), ((1, 0), [1])),
    "extend, repeated rows": (lambda e, s: e.extend(s[2], s, [1, 1, 0, 1]), lambda e, d: e.extend_device(d + N * K * M, d, N, K, [1, 1, 0, 1]),
                              ((3, 0), [2, 1])),
}


@pytest.mark.parametrize("entry", list(SCHEDULES))
def test_host_form_equals_device_form(eng, slab, dev, orc, entry):
    host, device, (cell, leaves) = SCHEDULES[entry]
    a, b = host(eng, slab), device(eng, dev.data_ptr())
    assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b)
    assert a[cell] == _card(orc, slab, leaves)
    if entry == "subsets":
        assert not a[0].any()
    if entry == "pairwise":
        assert np.array_equal(a, a.transpose(1, 0, 2))


def test_extend_takes_a_base_from_any_host_address(eng, slab):
    """16-byte alignment is a rule for a base in HBM only"""
    buf = np.zeros(K * M + 1, dtype=np.uint8)
    buf[1:] = slab[2].reshape(-1)
    assert buf[1:].ctypes.data % 16 and np.array_equal(eng.extend(buf[1:], slab), eng.extend(slab[2], slab))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nfixed", [0, 1])
def test_greedy_host_form_equals_device_form(eng, slab, dev, orc, mode, nfixed):
    cand = [1, 2, 0]
    order, card = eng.greedy(slab, KMIN, mode, cand, nfixed)
    order_d, card_d = eng.greedy_device(dev.data_ptr(), N, K, KMIN, mode, cand, nfixed)
    assert np.array_equal(order, order_d) and np.array_equal(card, card_d)
    assert sorted(order) == [0, 1, 2] and (not nfixed or order[0] == 1)
    assert card[0, 0] == _card(orc, slab, order[:1]) and card[2, 0] == _card(orc, slab, [0, 1, 2])
    first = [_card(orc, slab, [g]) for g in cand]
    if not nfixed:
        assert order[0] == cand[int(np.argmax(first) if mode == 0 else np.argmin(first))]


# ---------------------------------------------------------------------------------------------------------- the rules
def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _good(entry, leaf, out):
    """A good call of `entry` at (N, K): its arguments behind the context by name, in the ABI's order."""
    return {
        "card_batch": dict(regs=leaf, njobs=N * K, est=out),
        "hist_batch": dict(regs=leaf, njobs=N * K, hist=out),
        "progressive": dict(leaf=leaf, n=N, K=K, orderings=_i32(ORDS), norder=2, card=out),
        "pairwise": dict(leaf=leaf, n=N, K=K, card=out),
        "leave_out": dict(leaf=leaf, n=N, K=K, group=_i32(GROUPS), ngroups=2, card=out),
        "subsets": dict(leaf=leaf, n=N, K=K, card=out),
        "extend": dict(base=None, leaf=leaf, n=N, K=K, rows=_i32([0, 1, 2]), nrows=3, card=out),
        "greedy": dict(leaf=leaf, n=N, K=K, kmin=KMIN, mode=0, cand=_i32([0, 1, 2]), ncand=3, nfixed=0, nsteps=3,
                       order=np.zeros(3, dtype=np.int32), card=out),
    }[entry]


def _raw(eng, entry, suffix, leaf, over, ctx=True):
    """-> (return code, dd_last_error, the output buffer) of dd_<entry><suffix> called with _good's arguments, `over` laid over them"""
    out = np.full(256, -1.0)           # room for the largest result here, hist_batch's 6 x 64 words
    args = dict(_good(entry, leaf, out), **over)
    assert list(args) == list(_good(entry, leaf, out)), "an override names no argument of the entry"
    vals = [v.ctypes.data if isinstance(v, np.ndarray) else v for v in args.values()]
    rc = getattr(eng._lib, f"dd_{entry}{suffix}")(eng._ctx if ctx else None, *vals)
    return rc, eng._lib.dd_last_error().decode(), out


FORMS = ("", "_device")
SLAB = ("progressive", "pairwise", "leave_out", "subsets", "extend", "greedy")
RULES = [(e, dict(n=0), "outside 1..16" if e == "subsets" else "bad argument", FORMS) for e in SLAB]
RULES += [(e, dict(K=0), "bad argument", FORMS) for e in SLAB]
RULES += [(e, dict(leaf=None), "bad argument", FORMS) for e in SLAB]
RULES += [(e, dict(card=None), "bad argument", FORMS) for e in SLAB]
RULES += [
    ("card_batch", dict(njobs=-1), "bad argument", FORMS),
    ("card_batch", dict(regs=None), "bad argument", FORMS),
    ("card_batch", dict(est=None), "bad argument", FORMS),
    ("hist_batch", dict(njobs=-1), "bad argument", ("_device",)),
    ("hist_batch", dict(regs=None), "bad argument", ("_device",)),
    ("subsets", dict(n=17), "n=17 outside 1..16", FORMS),
    ("subsets", dict(n=17, K=0), "n=17 outside 1..16", FORMS),
    ("progressive", dict(orderings=_i32([[0, 1, 2], [2, N, 1]])), "ordering entry 3 outside 0..2", FORMS),
    ("progressive", dict(orderings=_i32([[0, -1, 2], [2, 0, 1]])), "ordering entry -1 outside 0..2", FORMS),
    ("progressive", dict(norder=0), "bad argument", FORMS),
    ("progressive", dict(orderings=None), "bad argument", FORMS),
    ("progressive", dict(n=0, orderings=_i32([[0, 9, 2], [2, 0, 1]])), "bad argument", FORMS),
    ("leave_out", dict(group=_i32([0, -1, 2])), r"group\[2\]=2 outside -1..1", FORMS),
    ("leave_out", dict(group=_i32([-2, 0, 1])), r"group\[0\]=-2 outside -1..1", FORMS),
    ("leave_out", dict(ngroups=0), "ngroups=0: at least one group", FORMS),
    ("leave_out", dict(ngroups=4), "ngroups=4 is more than the 3 leaves", FORMS),
    ("leave_out", dict(group=_i32([0, 0, 0]), ngroups=1), "group 0 holds every leaf", FORMS),
    ("leave_out", dict(group=None), "bad argument", FORMS),
    ("leave_out", dict(K=0, ngroups=0), "bad argument", FORMS),
    ("extend", dict(rows=_i32([]), nrows=0), "nrows=0: at least one row", FORMS),
    ("extend", dict(rows=_i32([0, N, 1])), r"rows\[1\]=3 outside 0..2", FORMS),
    ("extend", dict(rows=None, n=0), "bad argument", FORMS),
    ("extend", dict(base="leaf + 1"), "base must be 16-byte aligned", ("_device",)),
    ("extend", dict(base="leaf + 1", rows=_i32([0, N, 1])), r"rows\[1\]=3 outside 0..2", ("_device",)),
    ("greedy", dict(kmin=0), "k window 0..1 outside 1..64", FORMS),
    ("greedy", dict(cand=_i32([0, 1, 0])), "repeat", FORMS),
    ("greedy", dict(order=None), "bad argument", FORMS),
]


@pytest.mark.parametrize("entry,over,text,forms", RULES, ids=[f"{e}-{'-'.join(o)}-{i}" for i, (e, o, _, _) in enumerate(RULES)])
def test_argument_rules(engine_factory, slab, dev, entry, over, text, forms):
    """Every row is refused by the host with DD_EINVAL and these words, in the host form and in the device form alike, and
    leaves the output as it was."""
    eng = engine_factory(P, True)
    for suffix in forms:
        leaf = dev.data_ptr() if suffix else slab.ctypes.data
        o = {k: leaf + 1 if isinstance(v, str) else v for k, v in over.items()}
        rc, err, out = _raw(eng, entry, suffix, leaf, o)
        assert rc == EINVAL and re.search(text, err), (suffix, rc, err)
        assert (out == -1.0).all()


@pytest.mark.parametrize("entry", ["card_batch", "hist_batch", *SLAB])
def test_null_context(engine_factory, slab, dev, entry):
    eng = engine_factory(P, True)
    for suffix in FORMS if entry != "hist_batch" else ("_device",):
        rc, err, _ = _raw(eng, entry, suffix, dev.data_ptr() if suffix else slab.ctypes.data, {}, ctx=False)
        assert (rc, err) == (EINVAL, "null context"), suffix


def test_union_rules(engine_factory, slab, dev):
    eng = engine_factory(P, True)
    lib = eng._lib
    out = np.full(M, 99, dtype=np.uint8)
    for fn, ptrs, dst in ((lib.dd_union, [slab[g].ctypes.data for g in range(2)], out.ctypes.data),
                          (lib.dd_union_device, [dev[g].data_ptr() for g in range(2)], dev[N + 1].data_ptr())):
        arr = (C.c_void_p * 2)(*ptrs)
        for ctx, args, text in ((eng._ctx, (arr, 2, 24, dst), "len must be a multiple of 16"), (eng._ctx, (arr, 0, 16, dst), "bad argument"),
                                (eng._ctx, (None, 2, 16, dst), "bad argument"), (eng._ctx, (arr, 2, 16, None), "bad argument"),
                                (eng._ctx, (arr, 0, 24, dst), "bad argument"), (None, (arr, 2, 16, dst), "null context")):
            assert fn(ctx, *args) == EINVAL and lib.dd_last_error().decode() == text
    assert (out == 99).all()


def test_calls_that_are_no_errors(engine_factory, slab, dev):
    """No job is no error and touches nothing; null `rows` means every row whatever nrows says."""
    eng = engine_factory(P, True)
    for entry, suffix in (("card_batch", ""), ("card_batch", "_device"), ("hist_batch", "_device")):
        for over in (dict(njobs=0), dict(njobs=0, regs=None, **{"hist" if entry == "hist_batch" else "est": None})):
            rc, _, out = _raw(eng, entry, suffix, dev.data_ptr() if suffix else slab.ctypes.data, over)
            assert rc == 0 and (out == -1.0).all()
    want = eng.extend(None, slab)
    for suffix in FORMS:
        rc, err, out = _raw(eng, "extend", suffix, dev.data_ptr() if suffix else slab.ctypes.data, dict(rows=None, nrows=-5))
        assert rc == 0, err
        assert np.array_equal(out[:N * K].reshape(N, K), want) and (out[N * K:] == -1.0).all()


# ---------------------------------------------------------------------------------------------------------- the spans
SPANS = {"card_batch": 1, "progressive": 1, "pairwise": 1, "leave_out": 1, "subsets": 1, "extend, a base": 1, "extend, no base": 1,
         "extend, repeated rows": 1, "hist_batch": 1, "union": 1, "greedy": 5, "greedy, 2 of 3 steps": 3}


def test_span_counts(engine_factory, slab, dev):
    """DD_KERNEL_UNION spans of one call.  SPANS holds what dd_timing_read counted with the library built from the commit
    before the slab frame and the histogram step, both forms alike: one span around a schedule's launch; greedy one per
    step and one per update of the running union."""
    from dandd_amd.engine import KERNEL_UNION
    eng = engine_factory(P, True)
    d = dev.data_ptr()
    calls = {name: (lambda h=h: h(eng, slab), lambda g=g: g(eng, d)) for name, (h, g, _) in SCHEDULES.items()}
    calls["hist_batch"] = (lambda: eng.hist_batch_device(d, N * K),) * 2
    calls["union"] = (lambda: eng.union([slab[0], slab[1]]), lambda: eng.union_device([dev[0].data_ptr(), dev[1].data_ptr()], K * M, dev[N + 1].data_ptr()))
    calls["greedy"] = (lambda: eng.greedy(slab, KMIN, 0), lambda: eng.greedy_device(d, N, K, KMIN, 0))
    calls["greedy, 2 of 3 steps"] = (lambda: eng.greedy(slab, KMIN, 1, nfixed=1, nsteps=2), lambda: eng.greedy_device(d, N, K, KMIN, 1, nfixed=1, nsteps=2))
    eng.timing_enable(True)
    try:
        got = {}
        for name, forms in calls.items():
            counts = []
            for call in forms:
                eng.timing_reset()
                call()
                eng.synchronize()
                counts.append(eng.timing_read(KERNEL_UNION)[1])
            got[name] = counts
        print("DD_KERNEL_UNION spans per call (host form, device form):", got)
        assert got == {name: [c, c] for name, c in SPANS.items()}
    finally:
        eng.timing_reset()
        eng.timing_enable(False)
