"""What the ingestion pipeline's tests feed it, checked without a GPU: the draws of scripts/fuzz_ingest.py that
tests/test_gpu_fuzz.py runs, and the deterministic scenarios of tests/test_gpu_ingest.py (tests/ingest_worker.py).  No engine
runs here.  The shares below keep the sweep from quietly degenerating into single-batch calls: a generator that misses one
is to be changed, not the share."""
import os
import sys

import pytest

import ingest_worker as iw
from test_gpu_fuzz import FUZZ

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import fuzz_ingest  # noqa: E402


def test_the_sweeps_draws_make_many_batches_and_bind_the_window():
    (draws, seed), = [(row[1], row[2]) for row in FUZZ if row[0] == "fuzz_ingest.py"]
    assert seed == 512
    cfgs = list(fuzz_ingest.draws(draws, seed))
    assert len(cfgs) == draws
    three, beyond, kinds, mbs, missing = 0, 0, set(), set(), 0
    for cfg in cfgs:
        files = fuzz_ingest.build(cfg, seed)
        assert 1 <= len(files) <= 60 and sum(len(t) for _, _, t in files) <= fuzz_ingest.TEXT_CAP
        assert 1 <= cfg["kmin"] <= cfg["kmax"] <= 64 and cfg["kmax"] - cfg["kmin"] <= 2
        _, least, window = fuzz_ingest.guaranteed(cfg, files)
        three += least >= 3
        beyond += len(files) > window
        kinds |= {f["kind"] for f in cfg["files"]}
        mbs.add(cfg["batch_mb"])
        missing += cfg["missing_at"] is not None
    assert 2 * three >= draws, (three, draws)
    assert 4 * beyond >= draws, (beyond, draws)
    assert kinds == set(iw.KINDS)
    assert mbs == {1, 2, None}
    assert missing >= 4


@pytest.mark.parametrize("name", sorted(iw.SCENARIOS))
def test_the_scenarios_meet_their_own_conditions(name):
    """every deterministic scenario, for every nthreads it uses: a guaranteed batch count of 3 at least (F7: 2, by design of
    the call plan) and more files than the loaders' window (F7 excepted: seven files are fewer than two batches + a loader)"""
    for nthreads, nfiles, want, full, least, window in iw.conditions(name):
        assert least >= (2 if name == "F7" else 3), (nthreads, nfiles, want, least)
        if name != "F7":
            assert nfiles > window, (nthreads, nfiles, want, window)
    if name in ("A", "D"):
        assert iw.conditions(name)[0][4] >= 14          # more batches, of distinct shapes, than the 8 plan entries kept
        sizes = [len(t) for _, _, t in iw.files_of("A")]
        assert len(set(sizes)) == len(sizes) and sizes[0] > 5_000_000 and sizes[20] > 5_000_000
        plain = [s for i, s in enumerate(sizes) if i not in (0, 3, 4, 20)]      # (without the large and the tiny files: ascending)
        assert plain == sorted(plain)
    if name in iw.TAIL:
        sizes = [(n, len(d)) for n, d, _ in iw.files_of(name)]
        assert max(1, (1 << 20) // (sum(4 * n for _, n in sizes) // len(sizes))) == 3
        assert iw.want_of(sizes, 1) == (iw.TAIL[name][0], True)
        nthreads, nfiles, want, _, least, window = iw.conditions(name)[0]
        rem = nfiles - (least - 1) * want - want        # files that would be left behind the last full batch
        assert name == "F7" or 0 < rem < (want + 1) // 2                 # ... fewer than half a batch: the tail rule applies
        # F13: the last batch and its tail are within reach of the loaders (two batches in flight + nthreads files); F10: not
        assert name == "F7" or (want + rem <= nthreads) == (name == "F13")
