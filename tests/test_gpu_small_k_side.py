"""K1 launch structure of a big call (dd_sketch_api.hip: launch_classes): the small-k class (k <= 9: bitmap_kernel,
bitmap_finish_kernel) runs on one side lane beside the hashed classes, which stay back to back on the caller's stream, and the
lane is joined before the call returns.  bitmap_kernel reads the `complete` flags of its ks in one round trip (dd_sweep.hip).

DD_SIDE_JOBS=0 makes every call take the big-call structure, so the branch is reached with inputs of a megabase;
DD_NO_SIDE_SMALLK=1 keeps the small-k class on the caller's stream.  Registers must be the oracle's bit for bit either way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0xD4ADD
KMIN, KMAX = 4, 40
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

_INPUTS = {}
_WANT = {}


def _genomes(orc):
    """200 kbp in two records with a run of N across a line break, 70 kbp, 1 Mbp (more than one tile of 65536 tokens, and
    sizes that are no multiple of it)"""
    if "three" not in _INPUTS:
        a = orc.synth_fasta(SEED, 1, 200_000, 2).copy()
        seg = a[60_000:60_700]
        seg[np.isin(seg, ACGT)] = ord("N")
        _INPUTS["three"] = [a, orc.synth_fasta(SEED, 2, 70_000, 1), orc.synth_fasta(SEED, 3, 1_000_000, 3)]
    return _INPUTS["three"]


def _want(orc, name, fa, p, canonical):
    """the oracle's rows of k 4..40, computed once per (input, log2m, strand mode); a call over kmin..kmax wants a slice of it"""
    key = (name, p, canonical)
    if key not in _WANT:
        _WANT[key] = orc.sketch_sweep(fa, KMIN, KMAX, p, canonical)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _launch(torch, eng, bufs, fas, order, kmin, kmax, regs=None):
    """one dd_sketch_device call over bufs[i] for i in order, not waited for -> the device tensor [len(order)][K][m]"""
    if regs is None:
        regs = torch.empty((len(order), kmax - kmin + 1, eng.m), dtype=torch.uint8, device="cuda")
    eng.sketch_device([bufs[i].data_ptr() for i in order], [fas[i].size for i in order], kmin, kmax, regs.data_ptr())
    return regs


def _call(torch, eng, bufs, fas, order, kmin, kmax):
    regs = _launch(torch, eng, bufs, fas, order, kmin, kmax)
    eng.synchronize()
    return regs.cpu().numpy()


def _assert_rows(got, want, kmin, kmax, what):
    want = want[kmin - KMIN:kmax - KMIN + 1]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} registers differ, first at (k={kmin + bad[0][0]}, idx={bad[0][1]}): got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


def _big_call(monkeypatch, side_small_k=True):
    monkeypatch.setenv("DD_SIDE_JOBS", "0")
    if side_small_k:
        monkeypatch.delenv("DD_NO_SIDE_SMALLK", raising=False)
    else:
        monkeypatch.setenv("DD_NO_SIDE_SMALLK", "1")


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("p", [10, 14])
def test_big_call_structure_matches_the_oracle_and_the_control(engine_factory, torch_cuda, orc, monkeypatch, p, canonical):
    torch = torch_cuda
    eng = engine_factory(p, canonical)
    fas = _genomes(orc)
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    _big_call(monkeypatch)
    got = _call(torch, eng, bufs, fas, [0, 1, 2], KMIN, KMAX)
    for g, fa in enumerate(fas):
        _assert_rows(got[g], _want(orc, g, fa, p, canonical), KMIN, KMAX, f"genome {g}")
    _big_call(monkeypatch, side_small_k=False)
    control = _call(torch, eng, bufs, fas, [0, 1, 2], KMIN, KMAX)
    assert np.array_equal(got, control), "DD_NO_SIDE_SMALLK=1 gives other registers"


@pytest.mark.parametrize("kmin,kmax", [(10, 20), (4, 9), (9, 10)])
def test_k_ranges_round_the_class_boundary(engine_factory, torch_cuda, orc, monkeypatch, kmin, kmax):
    """10..20 has no small-k class and 4..9 nothing else: neither forks, and every class has a sweep span of its own.  9..10
    is the smallest call that forks: two classes, one span."""
    from dandd_amd.engine import KERNEL_SWEEP, plan_sweep
    torch = torch_cuda
    eng = engine_factory(14, True)
    fas = _genomes(orc)
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    classes = len(np.unique(plan_sweep(14, [f.size for f in fas], kmin, kmax)["kclass"]))
    assert classes == {(10, 20): 2, (4, 9): 1, (9, 10): 2}[(kmin, kmax)]
    _big_call(monkeypatch)
    eng.timing_enable(True)
    try:
        eng.timing_reset()
        got = _call(torch, eng, bufs, fas, [0, 1, 2], kmin, kmax)
        ms, spans = eng.timing_read(KERNEL_SWEEP)
    finally:
        eng.timing_reset()
        eng.timing_enable(False)
    assert spans == (1 if (kmin, kmax) == (9, 10) else classes) and ms > 0, (ms, spans)
    for g, fa in enumerate(fas):
        _assert_rows(got[g], _want(orc, g, fa, 14, True), kmin, kmax, f"genome {g}, k {kmin}..{kmax}")


def test_back_to_back_calls_wait_for_the_lane(engine_factory, torch_cuda, orc, monkeypatch):
    """Four calls on one context, nothing waited for in between, two k ranges and two output buffers in turn: every call zeroes
    the bitmaps and flags that the lane of the call before it may still be using, unless that lane was joined."""
    torch = torch_cuda
    eng = engine_factory(14, True)
    fas = _genomes(orc)
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    _big_call(monkeypatch)
    ranges = [(KMIN, KMAX), (7, 12)]
    outs = [torch.empty((3, k1 - k0 + 1, eng.m), dtype=torch.uint8, device="cuda") for k0, k1 in ranges]
    # every call's result is copied aside by a device copy on the engine's own stream: ordered behind the call and in front of
    # the next one, which overwrites the buffer two calls later, without the host waiting for anything
    snaps = [torch.empty_like(outs[i & 1]) for i in range(4)]
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for i in range(4):
        k0, k1 = ranges[i & 1]
        _launch(torch, eng, bufs, fas, [0, 1, 2], k0, k1, regs=outs[i & 1])
        snaps[i].copy_(outs[i & 1], non_blocking=True)
    eng.synchronize()
    torch.cuda.synchronize()
    for i, snap in enumerate(snaps):
        k0, k1 = ranges[i & 1]
        got = snap.cpu().numpy()
        for g, fa in enumerate(fas):
            _assert_rows(got[g], _want(orc, g, fa, 14, True), k0, k1, f"call {i}, genome {g}")


def test_complete_sets_and_flags(engine_factory, torch_cuda, orc, monkeypatch):
    """A uniform 1 Mbp genome has every canonical k-mer of k <= 7 within its first half: its flags go up mid-call.  A genome of
    A and C alone, as long, completes no set.  Both several times in one call: four times each (128 one-tile jobs, all resident
    at once), and twenty times each (640 jobs, more than the 512 that are resident together), so that the jobs of the last
    tiles start behind raised flags -- and, for A/C, behind flags that must have stayed down."""
    torch = torch_cuda
    p, kmax = 14, 12
    eng = engine_factory(p, True)
    uniform = _genomes(orc)[2]
    rng = np.random.default_rng(SEED)
    ac = np.concatenate([np.frombuffer(b">ac\n", dtype=np.uint8), ACGT[rng.integers(0, 2, 1_000_000)], np.frombuffer(b"\n", dtype=np.uint8)])
    for k in range(KMIN, 8):
        assert orc.exact_count([uniform[:uniform.size // 2]], k) == (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2, k
    assert orc.exact_count([ac], KMIN) < (4 ** KMIN + 4 ** (KMIN // 2)) // 2
    fas = [uniform, ac]
    want = [_want(orc, 2, uniform, p, True), orc.sketch_sweep(ac, KMIN, kmax, p, True)]
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    _big_call(monkeypatch)
    for copies in (4, 20):
        order = [0, 1] * copies
        got = _call(torch, eng, bufs, fas, order, KMIN, kmax)
        for g, i in enumerate(order):
            _assert_rows(got[g], want[i], KMIN, kmax, f"{copies} copies, genome {g} ({'uniform' if i == 0 else 'A/C only'})")


def test_timing_spans_of_a_big_call(engine_factory, torch_cuda, orc, monkeypatch):
    """A call that forks is timed as one span over the whole K1 phase; with the small-k class on the caller's stream every class
    has a span of its own, as big calls had before."""
    from dandd_amd.engine import KERNEL_SWEEP, plan_sweep
    torch = torch_cuda
    eng = engine_factory(14, True)
    fas = _genomes(orc)
    bufs = [torch.from_numpy(f.copy()).cuda() for f in fas]
    classes = len(np.unique(plan_sweep(14, [f.size for f in fas], KMIN, KMAX)["kclass"]))
    assert classes == 4      # k 4..9, 10..16, 17..32, 33..40
    eng.timing_enable(True)
    try:
        for side_small_k, spans in ((True, 1), (False, classes)):
            _big_call(monkeypatch, side_small_k)
            eng.timing_reset()
            _call(torch, eng, bufs, fas, [0, 1, 2], KMIN, KMAX)
            ms, n = eng.timing_read(KERNEL_SWEEP)
            assert n == spans and ms > 0, (side_small_k, ms, n)
    finally:
        eng.timing_reset()
        eng.timing_enable(False)
