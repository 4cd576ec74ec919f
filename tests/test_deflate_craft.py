"""CPU: the case table of tests/deflate_craft.py against zlib, WITHOUT the code under test -- the condition under which the
conformance tests of the two inflaters (test_inflate_conformance.py, test_gpu_inflate_conformance.py) mean anything.  Every valid
case inflates to exactly its intended text with nothing left over, zlib refuses every invalid one, every case's claims about its
own stream hold, and the containers are what gzip reads.  A case zlib and the writer disagree about is a bug in the writer."""
import gzip
import zlib

import pytest

import deflate_craft as dc


def zlib_inflate(data):
    """(text, whole: the stream ended at a final block's end, unused bytes) or zlib.error"""
    d = zlib.decompressobj(-15)
    text = d.decompress(data)
    return text, d.eof, d.unused_data


def test_the_table_covers_what_it_is_for():
    names = [c.name for c in dc.cases()]
    assert len(dc.invalid_cases()) >= 16
    for d in dc.OVERLAP_DISTS:
        assert "overlap_walk_d%d" % d in names and "overlap_place_d%d" % d in names
    copies = sum(len(dc.overlap_lengths(d)) * len(dc.OVERLAP_PHASES) for d in dc.OVERLAP_DISTS)
    assert 500 <= copies < 1000, copies
    assert set(dc.OVERLAP_DISTS) == set(range(1, 9)) | {31, 32, 33, 63, 64, 65, 127, 128, 129}
    assert sum(c.degenerate for c in dc.cases()) == 1


@pytest.mark.parametrize("case", dc.valid_cases(), ids=lambda c: c.name)
def test_valid_case_is_zlibs_text(case):
    s = case.stream()
    text, whole, unused = zlib_inflate(s.data)
    assert whole and unused == b"" and text == bytes(s.text), case.name
    assert len(s.data) == (s.bits + 7) // 8
    for what, claim in case.claims.items():
        assert claim(s), (case.name, what)
    # every block start the writer reports is one: zlib, given the text before it as its dictionary, reads the rest from there
    starts = s.starts if len(s.starts) <= 40 else s.starts[::7]
    for bit, at in starts:
        if bit % 8 == 0:
            d = zlib.decompressobj(-15, zdict=bytes(s.text[max(0, at - 32768):at]))
            assert d.decompress(s.data[bit // 8:]) == bytes(s.text[at:]), (case.name, bit)
    if case.bgzf:
        assert gzip.decompress(dc.bgzf_file([(s.data, bytes(s.text))])) == bytes(s.text)
    assert gzip.decompress(dc.gzip_member(s.data, bytes(s.text))) == bytes(s.text)


@pytest.mark.parametrize("case", dc.invalid_cases(), ids=lambda c: c.name)
def test_invalid_case_is_refused_by_zlib(case):
    s = case.stream()
    if "truncated" in case.claims:
        # (data that merely ends is no error to a streaming inflater: it waits for more.  What zlib does say: the stream is not whole;
        # in a container, where the trailer follows at once, it is refused like the others)
        text, whole, _ = zlib_inflate(s.data)
        assert not whole
    else:
        with pytest.raises(zlib.error):
            zlib_inflate(s.data)
    # the container's size fields, CRC-32 and ISIZE are those of the intended text: only the deflate data is at fault
    for data in (dc.bgzf_file([(s.data, bytes(s.text))]), dc.gzip_member(s.data, bytes(s.text))):
        with pytest.raises((zlib.error, OSError, EOFError)):
            gzip.decompress(data)
    block = dc.bgzf_block(s.data, bytes(s.text))
    assert int.from_bytes(block[16:18], "little") + 1 == len(block)
    assert block[-8:] == zlib.crc32(bytes(s.text)).to_bytes(4, "little") + len(s.text).to_bytes(4, "little")


def test_one_code_distance_tree_zlib_takes_one_bit_and_refuses_two():
    """the rule both decoders follow: an incomplete code is ONE code of ONE bit, nothing else"""
    body = dc._lits(dc.fasta(120, 600)) + [(10, 20)]
    ll = dc.lengths_for(dc.token_freqs(body)[0])
    lit = [ll.get(s, 0) for s in range(286)]
    good = dc.stream([dc.dynamic(body, lit, [0] * 8 + [1])])
    assert zlib_inflate(good.data)[0] == bytes(good.text)
    with pytest.raises(zlib.error, match="distances set"):
        zlib_inflate(dc.stream([dc.dynamic(body, lit, [0] * 8 + [2])]).data)


def test_concatenated_members_are_zlibs_text():
    """what the single-member tests feed the decoders: many cases' blocks in ONE stream, text blocks between them"""
    parts = [c.blocks for c in dc.valid_cases() if len(c.blocks) >= 2 and c.bgzf][:12]
    s = dc.concat_member(parts, 9000)
    text, whole, unused = zlib_inflate(s.data)
    assert whole and unused == b"" and text == bytes(s.text)
    assert gzip.decompress(dc.gzip_member(s.data, bytes(s.text))) == bytes(s.text)
