"""The multi-batch ingestion pipeline of dd_sketch_files (dandd_amd/csrc/dd_ingest.hip) against the oracle, per file: calls of
many batches (DD_BATCH_MB=1), more files than the loaders' window, more batch shapes than the plan cache keeps, device and
host buffers that grow while the other buffer set is in flight, a failing file deep inside a long call, promotion of the host
buffers to pinned memory, the six file kinds across batches, the tail rule of device-inflated calls, dd_sketch_fasta on both
sides of its 4 MiB switch, a caller-owned stream.  The scenarios and their conditions (guaranteed batch count, window) are in
tests/ingest_worker.py; tests/test_ingest_draws.py checks those conditions without a GPU.

Scenarios with more files than the window run in a child process with a time limit: a host-side deadlock of the loaders then
fails one test instead of blocking the suite.  The limit is no performance figure: the work is a few seconds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ingest_worker as iw

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ingest_dir(tmp_path_factory):
    """the scenarios' files and the oracle's registers for them: written once, shared by the module's tests and their children"""
    return str(tmp_path_factory.mktemp("ingest"))


CHILD = ["A-t1", "A-t2", "A-t16", "B-p17", "B-p18", "D-t1", "D-t3", "D-gz", "E", "F7", "F10", "F13"]


@pytest.mark.parametrize("scenario", CHILD)
def test_scenario_in_a_child(torch_cuda, ingest_dir, scenario):
    """A: 40 plain files, ascending then descending, 40 batches of 40 distinct shapes, edge files, two files larger than the
    batch budget, nthreads 1 / 2 / 16.  B: 24 files in batches of 4 at log2m 17 and 18 (the record path's areas grow mid-call).
    D: a missing path at index 25 / 0 / 39 (nthreads 1, 3) and a damaged .gz on the host decoder: the call raises, names the
    path and returns, the next call is right.  E: six file kinds, strict, registers and dd_inflate_files' text, then the host
    decoders.  F7 / F10 / F13: the tail rule, within and beyond the window.  Every one: registers == the oracle per file, batch count >= the guaranteed one,
    more files than the window (F7 excepted: a window holds two batches and seven files are fewer)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DD_")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "ingest_worker.py"), scenario, ingest_dir], capture_output=True, text=True,
                       timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == f"scenario {scenario}: ok"


def test_promotion_of_host_buffers(torch_cuda, ingest_dir, monkeypatch):
    """C: a fresh context's first call reads into pageable buffers, its second re-makes every buffer pinned under the running
    loaders, its third finds them pinned; a fourth call brings fewer and larger files.  All equal the oracle, 1-3 each other."""
    from dandd_amd.engine import Engine
    _, _, kmin, kmax, mb, _, _ = iw.SCENARIOS["A"]
    paths, sizes, _, ref = iw.ensure(ingest_dir, "A", 12, kmin, kmax)
    paths4, sizes4, _, ref4 = iw.ensure(ingest_dir, "C4", 12, kmin, kmax)
    want, full = iw.want_of(sizes, mb)
    monkeypatch.setenv("DD_BATCH_MB", str(mb))
    eng = Engine(device=0, log2m=12)
    try:
        calls = []
        for call in range(3):
            calls.append(eng.sketch_files(paths, kmin, kmax, nthreads=4))
            iw.check_batches(eng, len(paths), want, full, f"scenario C call {call + 1}")
        got4 = eng.sketch_files(paths4, kmin, kmax, nthreads=4)
        want4, full4 = iw.want_of(sizes4, mb)
        iw.check_batches(eng, len(paths4), want4, full4, "scenario C call 4")
    finally:
        eng.close()
    for call, got in enumerate(calls):
        assert np.array_equal(got, ref), (call, [i for i in range(len(paths)) if not np.array_equal(got[i], ref[i])])
    assert np.array_equal(calls[0], calls[1]) and np.array_equal(calls[1], calls[2])
    assert np.array_equal(got4, ref4), [i for i in range(len(paths4)) if not np.array_equal(got4[i], ref4[i])]


@pytest.mark.parametrize("nbytes", [(4 << 20) - 1, 4 << 20])
def test_sketch_fasta_on_both_sides_of_its_switch(engine_factory, orc, tmp_path, nbytes):
    """G: a plain file one byte short of 4 MiB takes dd_sketch_fasta's one read + one copy, one of 4 MiB the pipeline:
    sketch_fasta == sketch_buffer of the bytes == the oracle."""
    eng = engine_factory(14, True)
    fa = orc.synth_fasta(iw.SEED, 400, 4_300_000, 3)[:nbytes]
    assert fa.size == nbytes
    path = tmp_path / "switch.fasta"
    path.write_bytes(fa.tobytes())
    assert os.path.getsize(path) == nbytes
    want = orc.sketch_sweep(fa, 21, 22, 14)
    assert np.array_equal(eng.sketch_fasta(str(path), 21, 22), want)
    assert np.array_equal(eng.sketch_buffer(fa, 21, 22), want)


def test_zero_byte_file(engine_factory, tmp_path):
    """G: both entry points read an empty file as no k-mers at all"""
    eng = engine_factory(14, True)
    path = tmp_path / "empty.fasta"
    path.write_bytes(b"")
    one = eng.sketch_fasta(str(path), 21, 22)
    many = eng.sketch_files([str(path)], 21, 22)
    assert not one.any()
    assert np.array_equal(many[0], one)


def test_many_batches_on_a_caller_owned_stream(engine_factory, torch_cuda, ingest_dir, monkeypatch):
    """H: the pipeline orders its side streams against the context's stream, whichever that is"""
    _, _, kmin, kmax, mb, _, _ = iw.SCENARIOS["A"]
    paths, sizes, _, ref = iw.ensure(ingest_dir, "A", 12, kmin, kmax)
    want, full = iw.want_of(sizes, mb)
    iw.check_window(len(paths), 2, want, "scenario H")
    monkeypatch.setenv("DD_BATCH_MB", str(mb))
    eng = engine_factory(12, True)
    stream = torch_cuda.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    try:
        got = eng.sketch_files(paths, kmin, kmax, nthreads=2)
        iw.check_batches(eng, len(paths), want, full, "scenario H")
    finally:
        eng.set_stream(0)
    assert np.array_equal(got, ref), [i for i in range(len(paths)) if not np.array_equal(got[i], ref[i])]
