"""CPU: the host's piece decoder (dd_inflate.h: decode_piece, gunzip_member_parallel) on the crafted deflate streams of
tests/deflate_craft.py -- what libdeflate, pigz, zopfli and 7-zip may write and zlib's compressor never does -- as a stand-alone
program, tests/native/inflate_conformance.cpp, built under AddressSanitizer + UBSan where that build links and plain where it does
not.  The verdict on every stream is zlib's (tests/test_deflate_craft.py); "not applicable" passes nowhere: a valid stream must be
decoded to zlib's text, whole and from every block start without its history, an invalid one refused, and a mixed member of
several hundred KB must come out of gunzip_member_parallel with return value 1."""
import os
import re
import subprocess

import deflate_craft as dc
from dandd_amd.build import hipcc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dandd_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def mixed_member():
    """ONE member for gunzip_member_parallel: dynamic blocks of FASTA text, three in a row (a starting point for the block finder),
    and between them the blocks of crafted cases -- fixed blocks with matches, stored blocks, empty blocks of every type, copies at
    every overlap, codes of 15 bits.  Its pieces (min_piece 16 KiB, two and four threads) hold far more than 32 768 symbols each."""
    keep = ("all_length_codes_fixed", "all_distance_codes_fixed", "run_of_empty_stored_blocks", "run_of_empty_fixed_blocks",
            "run_of_empty_dynamic_blocks", "stored_behind_0_to_7_pad_bits", "stored_behind_partial_batches", "200_blocks_of_one_symbol",
            "block_start_at_every_bit_of_a_word", "copies_at_the_edges_of_the_history", "eob_alone_on_one_bit", "longest_symbol",
            "stair_literals", "long_distance_codes")
    parts = [c.blocks for c in dc.valid_cases() if c.name in keep or c.name.startswith("overlap_walk_d")]
    assert len(parts) == len(keep) + len(dc.OVERLAP_DISTS)
    return dc.concat_member(parts, 7000, text_bytes=5000)


def write_cases(d):
    lines = []
    for c in dc.cases():
        s = c.stream()
        (d / (c.name + ".deflate")).write_bytes(s.data)
        (d / (c.name + ".text")).write_bytes(bytes(s.text))
        lines.append(" ".join([c.name, "1" if c.valid else "0", str(s.bits), str(len(s.starts))] + ["%d:%d" % st for st in s.starts]))
    (d / "manifest").write_text("\n".join(lines) + "\n")
    m = mixed_member()
    assert len(m.data) > 200_000 and m.types.count(1) > 300 and m.types.count(0) > 80
    (d / "member.gz").write_bytes(dc.gzip_member(m.data, bytes(m.text)))
    (d / "member.text").write_bytes(bytes(m.text))


def build(exe, include=CSRC):
    base = [hipcc(), "-std=c++17", "-O1", "-g", "-Wall", "-I" + include, os.path.join(HERE, "native", "inflate_conformance.cpp"), "-o", exe,
            "-lz", "-lpthread"]
    b = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        print("sanitizer build failed, building plain:\n" + b.stderr[-1500:])
        b = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]


def test_host_decoder_follows_zlib_on_crafted_streams(tmp_path):
    d = tmp_path / "cases"
    d.mkdir()
    write_cases(d)
    exe = str(tmp_path / "inflate_conformance")
    build(exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(d)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "inflate_conformance: ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-6000:] + r.stderr[-4000:]
    m = re.search(r"cases (\d+) pieces (\d+) checks \d+ placeholders (\d+) w_min (-?\d+) w_max (-?\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    ncases, npieces, placeholders, w_min, w_max = map(int, m.groups())
    assert ncases == len(dc.cases()) and npieces >= 1000 and placeholders > 10_000
    # copies that reach exactly 32 768 bytes and exactly 1 byte in front of a piece were met (copies_at_the_edges_of_the_history)
    assert (w_min, w_max) == (0, 32767)
    assert len(re.findall(r"^member \d+ -> \d+ bytes, \d threads: 1$", r.stdout, re.M)) == 2
