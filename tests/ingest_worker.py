"""Helper of tests/test_gpu_ingest.py, tests/test_ingest_draws.py and scripts/fuzz_ingest.py: the named scenarios of the
ingestion pipeline's tests (dd_sketch_files, dandd_amd/csrc/dd_ingest.hip) -- their files, the batch size the pipeline's call
plan wants for them, the loaders' window -- and, as a program, one scenario run on an Engine of its own against the oracle:
    python tests/ingest_worker.py SCENARIO DIR      exit 0, or 1 with the first disagreement printed
Everything above run_scenario() needs no GPU: the CPU test checks the scenarios' conditions from it.
DIR keeps the scenario's files and the oracle's registers (computed once, shared by every test over the same files)."""
import gzip
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import dd_oracle as orc  # noqa: E402

SEED = 0x1D6E57
KINDS = ("fa", "gz", "gz2", "bgzf", "fq", "fqgz")   # plain FASTA, one gzip member, two members, BGZF, plain FASTQ, FASTQ as one member
NAMES = {"fa": "fasta", "gz": "fa.gz", "gz2": "fna.gz", "bgzf": "bgz.fa.gz", "fq": "fq", "fqgz": "fq.gz"}


def bgzf(raw, level=1, strategy=0, block=65280):
    """bgzip's container: <= 64 KiB gzip members with a 'BC' extra subfield that holds the member's size - 1, + the empty EOF block"""
    out = bytearray()
    for a in list(range(0, len(raw), block)) + [len(raw)]:
        part = raw[a:a + block] if a < len(raw) else b""
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        body = c.compress(part) + c.flush()
        out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(body) + 25).to_bytes(2, "little") + body +
                zlib.crc32(part).to_bytes(4, "little") + len(part).to_bytes(4, "little"))
    return bytes(out)


def fastq_text(seed, gi, nbases):
    """four-line FASTQ over synthetic bases: reads of 80-229 bases, every quality text as long as its read"""
    fa = orc.synth_fasta(seed, gi, nbases, 1).tobytes()
    bases = fa[fa.index(b"\n") + 1:].replace(b"\n", b"")
    out, at, r = [], 0, 0
    while at < len(bases):
        n = 80 + (r * 37) % 150
        s = bases[at:at + n]
        out.append(b"@r%d\n%s\n+\n%s\n" % (r, s, b"I" * len(s)))
        at += n
        r += 1
    return b"".join(out)


def container(kind, text, level=6):
    """the bytes on disk of `text` as one of KINDS (what `cat` / `zcat` prints of them is `text`)"""
    if kind in ("fa", "fq"):
        return text
    if kind in ("gz", "fqgz"):
        return gzip.compress(text, level)
    if kind == "gz2":
        cut = len(text) // 3
        return gzip.compress(text[:cut], level) + gzip.compress(text[cut:], 1)
    assert kind == "bgzf", kind
    return bgzf(text, level)


def make_file(kind, seed, gi, nbases, nrec=1, level=6):
    """(file name's suffix, bytes on disk, text) of one synthetic file"""
    text = fastq_text(seed, gi, nbases) if kind in ("fq", "fqgz") else orc.synth_fasta(seed, gi, nbases, nrec).tobytes()
    return NAMES[kind], container(kind, text, level), text


# ---------------------------------------------------------------------------- the call plan, restated (plan_call, dd_ingest.hip)
def default_batch_mb(log2m, any_gz, gpu_inflate):
    """the largest text per launch a call without DD_BATCH_MB may take (a context's first call at log2m >= 17 takes 128:
    the larger figure gives the smaller, always valid, bound on the batch count)"""
    return 512 if log2m >= 17 else (320 if any_gz and gpu_inflate else 128)


def want_of(files, batch_mb, gpu_inflate=True, log2m=12):
    """(files per batch the call plan wants, whether its batches are `full_batches`) for files = [(name, bytes on disk)];
    a .gz counts as 4 x its size; batch_mb None: DD_BATCH_MB unset"""
    nfiles = len(files)
    any_gz = any(name.endswith(".gz") and n > 0 for name, n in files)
    disk = sum((4 * n if name.endswith(".gz") else n) for name, n in files if n > 0)
    avg = max(1, disk // nfiles)
    mb = batch_mb if batch_mb else default_batch_mb(log2m, any_gz, gpu_inflate)
    want = max(1, min(256, (mb << 20) // avg))
    full = any_gz and gpu_inflate
    if full and nfiles >= 2:          # device-inflated calls: two batches at least, and equal ones
        nb = -(-nfiles // want)
        if nb == 3 and nfiles * 2 <= want * 5:
            nb = 2
        nb = max(nb, 2)
        want = -(-nfiles // nb)
    return want, full


def min_batches(nfiles, want, full):
    """The fewest launches the call can make: no batch holds more than `want` files -- except the LAST of a `full_batches` call,
    into which choose_batch folds a remainder of fewer than half a batch ((want + 1) // 2 - 1 files at most)."""
    tail = (want + 1) // 2 - 1 if full else 0
    return max(1, -(-(nfiles - tail) // want))


def window_of(nthreads, want):
    """files that may hold a host buffer at once (CallPlan::window)"""
    return max(nthreads + 2, 2 * want + nthreads)


# ---------------------------------------------------------------------------- the scenarios' files
def _edge(i, text):
    if i == 3:
        return b">x\n"                             # header only
    if i == 4:
        return b">y\nA\n"                          # one base
    if i == 11:
        return text.rstrip(b"\n")                  # no trailing newline
    if i == 17:
        return text.replace(b"\n", b"\r\n")        # CRLF line ends
    return text


def files_plain(nfiles, big=()):
    """Scenario A's list (B: its first 24 without the two large files): ascending, distinct sizes of 150 000 + 7 500 i bases,
    the edge files swapped in, and at the indices of `big` a 5 MB file (more than the whole batch budget; read in 2 MiB pieces
    at index 0 and in one 8 MiB piece at index 20)."""
    out = []
    for i in range(nfiles):
        nbases = 5_000_000 if i in big else 150_000 + 7_500 * i
        text = _edge(i, orc.synth_fasta(SEED, i, nbases, 1 + i % 3).tobytes())
        out.append((f"f{i:02d}.fasta", text, text))
    return out


def files_larger():
    """scenario C's fourth call: fewer and larger files"""
    return [(f"c{i}.fasta",) + 2 * (orc.synth_fasta(SEED, 100 + i, 900_000 + 100_000 * i, 2).tobytes(),) for i in range(5)]


def files_mixed(nfiles=24):
    """scenario E: the six kinds interleaved, ~400 KB of text each"""
    out = []
    for i in range(nfiles):
        kind = KINDS[i % 6]
        suffix, data, text = make_file(kind, SEED, 200 + i, (190_000 if kind in ("fq", "fqgz") else 380_000) + 3_000 * i, 1 + i % 2)
        out.append((f"e{i:02d}.{suffix}", data, text))
    return out


def files_bgzf(nfiles):
    """scenario F: BGZF files of ~0.3 MB of text: DD_BATCH_MB=1 takes three of them"""
    out = []
    for i in range(nfiles):
        text = orc.synth_fasta(SEED, 300 + i, 215_000 + 3_000 * i, 2).tobytes()
        out.append((f"b{i:02d}.fa.gz", bgzf(text, 6), text))
    return out


# name -> (files, log2m values, kmin, kmax, DD_BATCH_MB, nthreads values, gpu_inflate); what the CPU test checks, too
SCENARIOS = {
    "A": (lambda: files_plain(40, big=(0, 20)), (12,), 15, 17, 1, (1, 2, 16), True),
    "B": (lambda: files_plain(24), (17, 18), 20, 21, 1, (2, 8), True),
    "D": (lambda: files_plain(40, big=(0, 20)), (12,), 15, 17, 1, (1, 3), True),
    "E": (files_mixed, (12,), 15, 17, 1, (4,), True),
    "Ehost": (files_mixed, (12,), 15, 17, 1, (4,), False),
    "F7": (lambda: files_bgzf(7), (12,), 15, 17, 1, (1,), True),
    "F10": (lambda: files_bgzf(10), (12,), 15, 17, 1, (3,), True),
    "F13": (lambda: files_bgzf(13), (12,), 15, 17, 1, (4,), True),
}
FILES_OF = {"A": "A", "B": "B", "D": "A", "E": "E", "Ehost": "E", "F7": "F7", "F10": "F10", "F13": "F13", "C4": "C4"}   # scenarios that share files


_MADE = {}


def files_of(key):
    """the files of FILES_OF key: [(name, bytes on disk, text)], made once per process"""
    if key not in _MADE:
        _MADE[key] = files_larger() if key == "C4" else SCENARIOS[key][0]()
    return _MADE[key]


def conditions(name):
    """[(nthreads, nfiles, want, full, fewest batches, window)] of a scenario: the test's conditions on its own inputs"""
    _, _, _, _, mb, threads, gpu_inflate = SCENARIOS[name]
    sizes = [(n, len(data)) for n, data, _ in files_of(FILES_OF[name])]
    want, full = want_of(sizes, mb, gpu_inflate)
    return [(t, len(sizes), want, full, min_batches(len(sizes), want, full), window_of(t, want)) for t in threads]


def ensure(dirname, key, p, kmin, kmax):
    """the files of FILES_OF key under dirname/key (written once) and the oracle's registers [nfiles][K][m] (computed once);
    -> (paths, [(name, bytes on disk)], texts, oracle)"""
    d = os.path.join(dirname, key)
    os.makedirs(d, exist_ok=True)
    files = files_of(key)
    paths = []
    for name, data, _ in files:
        path = os.path.join(d, name)
        if not os.path.exists(path) or os.path.getsize(path) != len(data):
            with open(path + ".tmp", "wb") as f:
                f.write(data)
            os.replace(path + ".tmp", path)
        paths.append(path)
    ref = os.path.join(d, f"oracle_p{p}_k{kmin}_{kmax}.npy")
    if os.path.exists(ref):
        want = np.load(ref)
    else:
        want = np.stack([orc.sketch_sweep(np.frombuffer(text, np.uint8), kmin, kmax, p) for _, _, text in files])
        np.save(ref + ".tmp.npy", want)
        os.replace(ref + ".tmp.npy", ref)
    want.setflags(write=False)
    return paths, [(n, len(data)) for n, data, _ in files], [t for _, _, t in files], want


# ---------------------------------------------------------------------------- checks (these need an Engine)
class Disagreement(Exception):
    pass


def check_regs(got, want, what, order=None):
    for j in range(len(got)):
        i = order[j] if order is not None else j
        if not np.array_equal(got[j], want[i]):
            raise Disagreement(f"{what}: file {i} (position {j} of the call): {int((got[j] != want[i]).sum())} registers differ from the oracle's")


def check_batches(eng, nfiles, want, full, what):
    got, least = eng.last_ingest_stats()[2], min_batches(nfiles, want, full)
    print(f"{what}: {got} batches (at least {least}: {nfiles} files, {want} per batch)")
    if got < least:
        raise Disagreement(f"{what}: {got} batches, fewer than the {least} that {nfiles} files in batches of {want} need")
    return got


def check_window(nfiles, nthreads, want, what):
    if not nfiles > window_of(nthreads, want):
        raise Disagreement(f"{what}: {nfiles} files do not exceed the loaders' window of {window_of(nthreads, want)}")


def run_plain(eng, dirname, name, nthreads_list):
    """A / B: every file == the oracle, batch count and window conditions, then the same paths reversed on the same context"""
    _, _, kmin, kmax, mb, _, _ = SCENARIOS[name]
    paths, sizes, _, ref = ensure(dirname, FILES_OF[name], eng.log2m, kmin, kmax)
    want, full = want_of(sizes, mb)
    os.environ["DD_BATCH_MB"] = str(mb)
    for t in nthreads_list:
        what = f"scenario {name} log2m {eng.log2m} nthreads {t}"
        check_window(len(paths), t, want, what)
        check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=t), ref, what)
        check_batches(eng, len(paths), want, full, what)
        back = list(range(len(paths)))[::-1]
        check_regs(eng.sketch_files([paths[i] for i in back], kmin, kmax, nthreads=t), ref, what + " reversed", back)
        check_batches(eng, len(paths), want, full, what + " reversed")


def run_failing(eng, dirname, nthreads):
    """D: a missing path at index 25, 0, 39: the call raises and names it; the next call over the intact list == the oracle"""
    from dandd_amd.engine import EngineError
    _, _, kmin, kmax, mb, _, _ = SCENARIOS["D"]
    paths, sizes, _, ref = ensure(dirname, "A", eng.log2m, kmin, kmax)
    want, full = want_of(sizes, mb)
    os.environ["DD_BATCH_MB"] = str(mb)
    check_window(len(paths), nthreads, want, "scenario D")
    for at in (25, 0, 39):
        what = f"scenario D nthreads {nthreads} missing at {at}"
        nope = os.path.join(dirname, f"no_such_file_{at}.fasta")
        broken = paths[:at] + [nope] + paths[at + 1:]
        try:
            eng.sketch_files(broken, kmin, kmax, nthreads=nthreads)
        except EngineError as e:
            if nope not in str(e):
                raise Disagreement(f"{what}: the error does not name the path: {e}")
        else:
            raise Disagreement(f"{what}: the call did not raise")
        check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=nthreads), ref, what + ", the next call")
        check_batches(eng, len(paths), want, full, what + ", the next call")


def run_truncated(eng, dirname, nthreads=3):
    """D: a truncated, damaged .gz at index 25 read by the host decoder (DD_NO_GPU_INFLATE=1): its error comes through the same drain"""
    from dandd_amd.engine import EngineError
    _, _, kmin, kmax, mb, _, _ = SCENARIOS["D"]
    paths, sizes, texts, ref = ensure(dirname, "A", eng.log2m, kmin, kmax)
    cut = os.path.join(dirname, "truncated.fa.gz")
    # (A .gz that merely ENDS early is no error to zlib's gzread, which the host decoder follows: it hands out what was decoded,
    # scripts/fuzz_damage.py.  So the truncated file also has 64 damaged bytes in its deflate data, which gzread refuses.)
    whole = bytearray(gzip.compress(texts[25], 6))
    whole[len(whole) // 2:len(whole) // 2 + 64] = b"\xff" * 64
    whole = bytes(whole[:len(whole) - 1000])
    try:
        zlib.decompressobj(31).decompress(whole)
        raise Disagreement("scenario D truncated .gz: zlib reads the damaged file")
    except zlib.error:
        pass
    with open(cut, "wb") as f:
        f.write(whole)
    os.environ["DD_BATCH_MB"] = str(mb)
    os.environ["DD_NO_GPU_INFLATE"] = "1"
    try:
        broken = paths[:25] + [cut] + paths[26:]
        try:
            eng.sketch_files(broken, kmin, kmax, nthreads=nthreads)
        except EngineError as e:
            if cut not in str(e):
                raise Disagreement(f"scenario D truncated .gz: the error does not name the path: {e}")
        else:
            raise Disagreement("scenario D truncated .gz: the call did not raise")
        want, full = want_of(sizes, mb, gpu_inflate=False)
        check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=nthreads), ref, "scenario D truncated .gz, the next call")
        check_batches(eng, len(paths), want, full, "scenario D truncated .gz, the next call")
    finally:
        del os.environ["DD_NO_GPU_INFLATE"]


def run_mixed(eng, dirname):
    """E: six kinds over many batches, strict: registers == the oracle, dd_inflate_files == the text; then the host decoders"""
    _, _, kmin, kmax, mb, (t,), _ = SCENARIOS["E"]
    paths, sizes, texts, ref = ensure(dirname, "E", eng.log2m, kmin, kmax)
    os.environ.update(DD_BATCH_MB=str(mb), DD_GUNZIP_MIN_KB="1", DD_INFLATE_STRICT="1")
    want, full = want_of(sizes, mb)
    check_window(len(paths), t, want, "scenario E")
    check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=t), ref, "scenario E")
    check_batches(eng, len(paths), want, full, "scenario E")
    got = eng.inflate_files(paths, nthreads=t)
    check_batches(eng, len(paths), want, full, "scenario E inflate_files")
    for i, (g, text) in enumerate(zip(got, texts)):
        if KINDS[i % 6] not in ("fq", "fqgz") and g.tobytes() != text:      # (FASTQ: the text is rewritten for K0)
            raise Disagreement(f"scenario E: inflate_files: file {i} ({paths[i]}): {len(g)} bytes that are not the file's text ({len(text)})")
    os.environ["DD_NO_GPU_INFLATE"] = "1"
    try:
        want, full = want_of(sizes, mb, gpu_inflate=False)
        check_window(len(paths), t, want, "scenario E, host decoders")
        check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=t), ref, "scenario E, host decoders")
        check_batches(eng, len(paths), want, full, "scenario E, host decoders")
    finally:
        del os.environ["DD_NO_GPU_INFLATE"]


TAIL = {"F7": (4, 3), "F10": (3, None), "F13": (3, 4)}     # files per batch the plan wants, most batches the call may make


def run_tail(eng, dirname, name):
    """F: BGZF files, 3 per MB, the tail rule of device-inflated calls.
    F7: the plan makes two batches of 4 of 7 files (at most 3 launches).
    F13, four loaders: 3 + 3 + 3 + 3 would leave one file, fewer than half a batch: it joins the fourth batch: 4 launches.
    F10, three loaders: 3 + 3 + 3 would leave one file as well, but file 9 lies beyond the loaders' window of 9 until the first
    batch is retired, which is after the third batch is chosen: choose_batch used to wait for it for ever (found by this
    scenario).  The call returns, with a small last batch.
    (A batch leaves with the files that are loaded after 3 ms: the count is looked at on the context's second call, whose
    loaders find their buffers and the files' pages in place; the first call's registers are checked like the second's.)"""
    _, _, kmin, kmax, mb, (t,), _ = SCENARIOS[name]
    paths, sizes, _, ref = ensure(dirname, name, eng.log2m, kmin, kmax)
    os.environ.update(DD_BATCH_MB=str(mb), DD_INFLATE_STRICT="1")
    first = max(1, (mb << 20) // (sum(4 * n for _, n in sizes) // len(sizes)))
    want, full = want_of(sizes, mb)
    if first != 3 or not full or want != TAIL[name][0]:
        raise Disagreement(f"scenario {name}: the plan wants {first} then {want} files per batch, not 3 then {TAIL[name][0]}")
    if name != "F7":
        check_window(len(paths), t, want, f"scenario {name}")
    for call in (1, 2):
        check_regs(eng.sketch_files(paths, kmin, kmax, nthreads=t), ref, f"scenario {name} call {call}")
        got = check_batches(eng, len(paths), want, full, f"scenario {name} call {call}")
    if TAIL[name][1] is not None and got > TAIL[name][1]:
        raise Disagreement(f"scenario {name}: more than {TAIL[name][1]} batches")


def run_scenario(scenario, dirname):
    from dandd_amd.engine import Engine
    name, _, arg = scenario.partition("-")
    log2m = int(arg[1:]) if name == "B" else 12
    with Engine(device=0, log2m=log2m) as eng:
        if name in ("A", "B"):
            run_plain(eng, dirname, name, [int(arg[1:])] if name == "A" else list(SCENARIOS["B"][5]))
        elif name == "D":
            run_truncated(eng, dirname) if arg == "gz" else run_failing(eng, dirname, int(arg[1:]))
        elif name == "E":
            run_mixed(eng, dirname)
        elif name in TAIL:
            run_tail(eng, dirname, name)
        else:
            raise SystemExit(f"unknown scenario {scenario}")


def main():
    scenario, dirname = sys.argv[1], sys.argv[2]
    try:
        run_scenario(scenario, dirname)
    except Disagreement as e:
        print(f"DISAGREEMENT {e}")
        sys.exit(1)
    print(f"scenario {scenario}: ok")


if __name__ == "__main__":
    main()
