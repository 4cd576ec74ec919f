"""GPU: the device inflate (dd_deflate.h, dd_ginflate.hip, dd_gunzip.hip) on the crafted deflate streams of tests/deflate_craft.py
-- what libdeflate, pigz, igzip, zopfli and 7-zip may write and zlib's compressor never does: 15-bit codes on the frequent
symbols, every spelling of every length and distance, copies at every overlap and batch phase, block starts at every bit of a
word, runs of empty blocks, odd dynamic headers.  The reference for every byte is Python's zlib (tests/test_deflate_craft.py
pins the table to it); every comparison is equality.  Valid streams run with DD_INFLATE_STRICT=1: a block the device declines
fails the test instead of going to the host decoder.  Invalid streams must raise, because zlib raises on every one."""
import copy
import zlib

import numpy as np
import pytest

import deflate_craft as dc

pytestmark = pytest.mark.gpu

KMIN, KMAX = 19, 21
FILES = 6


def _good_block(seed):
    """a plain block of text in front of a file's crafted ones: the ingestion looks into a file's first bytes (FASTQ or FASTA?)
    with zlib, and a first block that is unusual would route the whole file to the host"""
    body = dc.fasta(600, seed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(body) + co.flush(), body


def bgzf_files_of_valid_cases():
    """[(name, bytes on disk, text)]: the valid cases that fit a BGZF block, one per block, dealt over FILES files"""
    per = [[_good_block(800 + i)] for i in range(FILES)]
    for i, c in enumerate(c for c in dc.valid_cases() if c.bgzf):
        s = c.stream()
        per[i % FILES].append((s.data, bytes(s.text)))
    return [("valid%d.fa.gz" % i, dc.bgzf_file(blocks), b"".join(t for _, t in blocks)) for i, blocks in enumerate(per)]


def members_of_valid_cases():
    """[(name, bytes on disk, text)]: the valid cases of two blocks and more as parts of three single gzip members, dynamic text
    blocks between them (the finder's starts)"""
    multi = [c for c in dc.valid_cases() if len(c.blocks) >= 2]
    out = []
    for i in range(3):
        s = dc.concat_member([c.blocks for c in multi[i::3]], 8100 + 100 * i)
        assert len(s.data) >= 4 * 16384
        out.append(("member%d.fa.gz" % i, dc.gzip_member(s.data, bytes(s.text)), bytes(s.text)))
    return out


def _zlib_text(data):
    """the file's text by zlib, member after member (gzip.decompress does the same; this one says where it stopped)"""
    out, rest = [], data
    while rest.strip(b"\0"):
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def _write(tmp_path, files):
    paths = []
    for name, data, _ in files:
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    return paths


def test_bgzf_valid_cases_strict(engine_factory, tmp_path, monkeypatch):
    eng = engine_factory(14, True)
    files = bgzf_files_of_valid_cases()
    paths = _write(tmp_path, files)
    for name, data, text in files:
        assert _zlib_text(data) == text, name
    want = [eng.sketch_buffer(np.frombuffer(text, np.uint8), KMIN, KMAX) for _, _, text in files]
    monkeypatch.setenv("DD_INFLATE_STRICT", "1")
    texts = eng.inflate_files(paths)
    got = eng.sketch_files(paths, KMIN, KMAX)
    monkeypatch.delenv("DD_INFLATE_STRICT")
    assert eng.last_ingest_stats()[2] >= 1
    for (name, _, text), t in zip(files, texts):
        tb = t.tobytes()
        if tb != text:
            first = next((i for i in range(min(len(tb), len(text))) if tb[i] != text[i]), min(len(tb), len(text)))
            raise AssertionError(f"{name}: {len(tb)} bytes for {len(text)}, first difference at {first}")
    for (name, _, _), g, w in zip(files, got, want):
        assert np.array_equal(g, w), name
    monkeypatch.setenv("DD_NO_GPU_INFLATE", "1")                 # the host decoders on the same files: same registers
    host = eng.sketch_files(paths, KMIN, KMAX)
    monkeypatch.delenv("DD_NO_GPU_INFLATE")
    for (name, _, _), g, w in zip(files, host, want):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("guess_kb", ["4", "32"])
def test_single_member_valid_cases_strict(engine_factory, tmp_path, monkeypatch, guess_kb):
    """the crafted symbols through inflate_kernel<3>, placeholders and the arena modes"""
    eng = engine_factory(14, True)
    files = members_of_valid_cases()
    paths = _write(tmp_path, files)
    for name, data, text in files:
        assert _zlib_text(data) == text, name
    want = [eng.sketch_buffer(np.frombuffer(text, np.uint8), KMIN, KMAX) for _, _, text in files]
    monkeypatch.setenv("DD_GUNZIP_MIN_KB", "16")
    monkeypatch.setenv("DD_GUNZIP_GUESS_KB", guess_kb)
    monkeypatch.setenv("DD_INFLATE_STRICT", "1")
    texts = eng.inflate_files(paths)
    got = eng.sketch_files(paths, KMIN, KMAX)
    for (name, _, text), t in zip(files, texts):
        tb = t.tobytes()
        if tb != text:
            first = next((i for i in range(min(len(tb), len(text))) if tb[i] != text[i]), min(len(tb), len(text)))
            raise AssertionError(f"{name}: {len(tb)} bytes for {len(text)}, first difference at {first}")
    for (name, _, _), g, w in zip(files, got, want):
        assert np.array_equal(g, w), name


def invalid_files():
    """[(name, bytes on disk, intended text)]: every invalid case as a BGZF file -- a good block, the case's block, the EOF block -- and, where the
    fault does not depend on the block standing alone, as a single member of > 16 KiB: text blocks, the case's blocks, a stored block"""
    out = []
    head = dc.Stream()
    for i in range(3):
        head.add(dc.member_text_block(head, 6000, 8500 + i), False)
    tail = dc.fasta(14000, 8600)
    for c in dc.invalid_cases():
        s = c.stream()
        out.append((c.name + ".bgzf.fa.gz", dc.bgzf_file([_good_block(900), (s.data, bytes(s.text))]), _good_block(900)[1] + bytes(s.text)))
        if c.name in ("invalid_distance_before_the_text", "invalid_distance_one_before_the_text", "invalid_ends_before_end_of_block"):
            continue            # (in a member the copy finds text in front of it; a stream that stops goes on with what follows)
        m = copy.deepcopy(head)
        for b in c.blocks:
            m.add(b, False)
        m.add(dc.stored(tail), False)
        m.add(dc.fixed(list(b"ACGT\n")), True)
        assert len(m.data) + 18 >= 16384
        out.append((c.name + ".member.fa.gz", dc.gzip_member(m.data, bytes(m.text)), bytes(m.text)))
    return out


# What libdeflate (the host's serial decoder where the machine has it, dd_io.h) reads although zlib refuses it: a repeat that runs
# beyond HLIT + HDIST, HLIT 287, HDIST 31 -- it makes the intended text of them, so CRC-32 and ISIZE agree.  The device
# refuses all three; behind it these cases raise with zlib as the host's decoder (DD_NO_LIBDEFLATE=1, a process of its own: the
# library is looked up once per process) and may, with libdeflate, give the registers of the intended text -- never other ones.
LIBDEFLATE_READS = ("invalid_run_beyond_hlit_plus_hdist", "invalid_hlit_287", "invalid_hdist_31")
REFUSED = "refused by the device decoder"

CHILD = """
import sys
from dandd_amd.engine import Engine, EngineError
sketched = []
for path in sys.argv[1:]:
    with Engine(device=0, log2m=14, canonical=True) as eng:
        try:
            eng.sketch_files([path], %d, %d)
            sketched.append(path)
        except EngineError:
            pass
print("SKETCHED", sketched)
sys.exit(1 if sketched else 0)
""" % (KMIN, KMAX)


def test_invalid_cases_are_refused(torch_cuda, tmp_path, monkeypatch):
    """zlib refuses every one of them (checked here again, on the files themselves).  Strict mode: the DEVICE decoder refuses the
    block or piece itself.  Then without it: the call raises, the host decoder has the last word.  A fresh context after each
    refusal (three refusals keep one on the host); at the end a good crafted file still decodes on the device."""
    import gzip
    import os
    import subprocess
    import sys
    from dandd_amd.engine import Engine, EngineError
    monkeypatch.setenv("DD_GUNZIP_MIN_KB", "16")
    files = invalid_files()
    assert len(files) == 2 * len(dc.invalid_cases()) - 3 and len(dc.invalid_cases()) >= 16
    wrong, lenient = [], []
    eng = Engine(device=0, log2m=14, canonical=True)
    try:
        for name, data, text in files:
            with pytest.raises((zlib.error, OSError, EOFError)):
                gzip.decompress(data)
            path = tmp_path / name
            path.write_bytes(data)
            monkeypatch.setenv("DD_INFLATE_STRICT", "1")
            try:
                eng.sketch_files([str(path)], KMIN, KMAX)
                wrong.append((name, "the device decoder takes it"))
            except EngineError as e:
                if REFUSED not in str(e):
                    wrong.append((name, "strict mode: " + str(e)))
            monkeypatch.delenv("DD_INFLATE_STRICT")
            try:
                regs = eng.sketch_files([str(path)], KMIN, KMAX)[0]
                if name.split(".")[0] not in LIBDEFLATE_READS:
                    wrong.append((name, "sketched although zlib refuses it"))
                elif not np.array_equal(regs, eng.sketch_buffer(np.frombuffer(text, np.uint8), KMIN, KMAX)):
                    wrong.append((name, "sketched, and not as the intended text"))
                else:
                    lenient.append(str(path))
            except EngineError:
                pass
            eng.close()
            eng = Engine(device=0, log2m=14, canonical=True)
        assert not wrong, wrong
        good = bgzf_files_of_valid_cases()[0]
        (tmp_path / good[0]).write_bytes(good[1])
        monkeypatch.setenv("DD_INFLATE_STRICT", "2")
        assert eng.inflate_files([str(tmp_path / good[0])])[0].tobytes() == good[2]
    finally:
        eng.close()
    if lenient:     # the same files with zlib behind the device decoder
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, DD_NO_LIBDEFLATE="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        env.pop("DD_INFLATE_STRICT", None)
        r = subprocess.run([sys.executable, "-c", CHILD] + lenient, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_valid_files_do_reach_the_device_decoder(engine_factory, tmp_path, monkeypatch):
    """The condition under which the strict tests above mean what they say: the files they use are decoded on the device, not
    routed to the host before it.  The same files with ONE bit of the last block's CRC-32 flipped are refused BY THE DEVICE."""
    from dandd_amd.engine import EngineError
    eng = engine_factory(14, True)
    monkeypatch.setenv("DD_GUNZIP_MIN_KB", "16")
    monkeypatch.setenv("DD_INFLATE_STRICT", "1")
    for name, data, _ in bgzf_files_of_valid_cases() + members_of_valid_cases():
        at = len(data) - 8 - (len(dc.BGZF_EOF) if name.startswith("valid") else 0)
        bad = bytearray(data)
        bad[at] ^= 1
        path = tmp_path / ("crc_" + name)
        path.write_bytes(bytes(bad))
        with pytest.raises(EngineError, match=REFUSED):
            eng.sketch_files([str(path)], KMIN, KMAX)


def test_one_distance_code_of_two_bits_is_refused_by_the_device(engine_factory, tmp_path, monkeypatch):
    """The block zlib answers "invalid distances set" to -- one distance code, of two bits, used; CRC-32 and ISIZE those of the text a
    lenient decoder makes of it (the parent of this test sketched it) -- is refused by the DEVICE decoder itself, while the same
    block with the code on one bit is decoded there."""
    from dandd_amd.engine import EngineError
    eng = engine_factory(14, True)
    body = list(dc.fasta(120, 600)) + [(10, 20)] + list(dc.fasta(300, 601))
    ll = dc.lengths_for(dc.token_freqs(body)[0])
    lit = [ll.get(s, 0) for s in range(286)]
    monkeypatch.setenv("DD_INFLATE_STRICT", "1")
    for bits in (1, 2):
        s = dc.stream([dc.dynamic(body, lit, [0] * 8 + [bits])])
        path = tmp_path / ("one_code_%d.fa.gz" % bits)
        path.write_bytes(dc.bgzf_file([_good_block(901), (s.data, bytes(s.text))]))
        if bits == 1:
            assert eng.inflate_files([str(path)])[0].tobytes() == _good_block(901)[1] + bytes(s.text)
        else:
            with pytest.raises(EngineError, match=REFUSED):
                eng.inflate_files([str(path)])
