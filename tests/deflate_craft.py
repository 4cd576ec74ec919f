"""A deflate WRITER for the tests of the two inflaters (dd_deflate.h / dd_ginflate.hip / dd_gunzip.hip on the device, dd_inflate.h on the
host): raw deflate (RFC 1951) from an explicit description -- which block types, which code lengths, which symbols, how a length
is spelled, how the dynamic header's length list is run-length coded -- so that the decoders meet what zlib's compressor never
writes but libdeflate, pigz, igzip, zopfli and 7-zip may.  Plain Python, no native code; nothing under dandd_amd/ imports it.

The writer chooses nothing by itself: every default below is the output of one of the named helpers (lengths_for, rle_greedy,
complete_lens), which a caller may replace.  For every stream it returns the intended text, the bit and text position of every
block start, the positions a case marked, and figures about the codes that were used (Stream.facts).

cases() is the ONE table all tests share (tests/test_deflate_craft.py checks every entry against zlib, without the code under
test: a case zlib and this writer disagree about is a bug here, not a finding).  Shapes are the smallest at which the decoders' units
can go wrong: 64-byte output batches, 64-bit symbol windows, 32-bit words in windows of 64, 10-bit tables, 32 768 bytes of history,
text_crc's split from 8192 bytes on.  Texts are FASTA-like (a '>' line, then ACGT and newlines)."""
import heapq
import random
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EOB = 256
FAST = 10                      # the decoders' table bits: a longer code goes through their slow paths
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# ---------------------------------------------------------------------------- bits and codes
class BitWriter:
    """bits go out LSB first (RFC 1951, 3.1.1); Huffman codes arrive already reversed (canonical())"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.pos = 0            # bits written

    def bits(self, value, k):
        self.acc |= (value & ((1 << k) - 1)) << self.n
        self.n += k
        self.pos += k
        if self.n >= 32:
            while self.n >= 8:
                self.out.append(self.acc & 255)
                self.acc >>= 8
                self.n -= 8

    def align(self, fill=0):
        """to the byte boundary; the pad bits carry `fill`'s low bits (an inflater ignores them)"""
        k = -self.pos % 8
        self.bits(fill, k)
        return k

    def getvalue(self):
        out, acc, n = bytearray(self.out), self.acc, self.n
        while n > 0:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
        return bytes(out)


def canonical(lengths):
    """[(code reversed for LSB-first output, length) or None] per symbol: RFC 1951, 3.2.2.  Lengths that are no code (oversubscribed)
    still get the bits the algorithm gives them, cut to their length: such a header is written to be refused."""
    key = tuple(lengths)
    if key not in _CANONICAL:
        _CANONICAL[key] = _canonical(key)
    return _CANONICAL[key]


_CANONICAL = {}


def _canonical(lengths):
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - l) for l in lengths if l)


def lengths_for(freq, maxbits=15):
    """Huffman code lengths for {symbol: count > 0}: two symbols at least, none longer than maxbits (counts are halved until it fits)"""
    assert len(freq) >= 2
    freq = dict(freq)
    while True:
        heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
        heapq.heapify(heap)
        depth = dict.fromkeys(freq, 0)
        while len(heap) > 1:
            fa, sa, a = heapq.heappop(heap)
            fb, sb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(sa, sb), a + b))
        if max(depth.values()) <= maxbits:
            return depth
        freq = {s: f // 2 + 1 for s, f in freq.items()}


def complete_lens(wanted, n, pool):
    """a COMPLETE code of n symbols that gives `wanted` ({symbol: length}) what it asks and spends the rest of the code space on
    symbols of `pool` (which the case never uses), largest pieces first"""
    lens = [0] * n
    for s, l in wanted.items():
        lens[s] = l
    rest = 32768 - kraft(lens)
    assert rest >= 0, "the wanted lengths are oversubscribed"
    pool = [s for s in pool if s not in wanted]
    for l in range(1, 16):
        while rest >= 1 << (15 - l):
            lens[pool.pop(0)] = l
            rest -= 1 << (15 - l)
    assert kraft(lens) == 32768
    return lens


def length_symbol(length, spelling=None):
    """(symbol, extra value, extra bits); 258 is symbol 285, or -- spelling '284+31', which RFC 1951 allows and zlib never writes --
    284 with all five extra bits set"""
    if length == 258:
        return (284, 31, 5) if spelling == "284+31" else (285, 0, 0)
    i = max(j for j in range(28) if LEN_BASE[j] <= length)
    assert length - LEN_BASE[i] < 1 << LEN_EXTRA[i], length
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def dist_symbol(dist):
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    assert 1 <= dist <= 32768 and dist - DIST_BASE[i] < 1 << DIST_EXTRA[i], dist
    return i, dist - DIST_BASE[i], DIST_EXTRA[i]


# ---------------------------------------------------------------------------- the run-length coding of a dynamic header's lengths
def rle_plain(lens):
    """one code-length symbol per length, no 16 / 17 / 18"""
    return list(lens)


def rle_greedy(lens):
    """zlib-like: zeros by 18 / 17, repeats of a length by 16; an op is a length 0..15 or (16 | 17 | 18, repeat count)"""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                ops.append((18, min(run, 138)))
                run -= min(run, 138)
            if run >= 3:
                ops.append((17, run))
                run = 0
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                ops.append((16, min(run, 6)))
                run -= min(run, 6)
        ops += [v] * run
        i = j
    return ops


def rle_expand(ops):
    """the length list the ops stand for (what an inflater reads out of them)"""
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            out += [out[-1] if op[0] == 16 else 0] * op[1]
    return out


# ---------------------------------------------------------------------------- blocks
# A token is a literal (int 0..255), a copy (length, distance) or (length, distance, '284+31'), or one of
#   ('mark', key)                      the bit and text position here go to Stream.marks[key]
#   ('litsym', s)                      literal/length symbol s as it is (286, 287: no inflater may take them)
#   ('distsym', length, ds, v, k)      the length, then distance symbol ds as it is with k extra bits of value v
#   ('bits', v, k)                     k bits
def stored(data, final=False, pad=0, nlen=None):
    return dict(type=0, final=final, data=bytes(data), pad=pad, nlen=nlen)


def fixed(tokens, final=False, eob=True):
    return dict(type=1, final=final, tokens=list(tokens), eob=eob)


def dynamic(tokens, lit_lens, dist_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, ops=None, eob=True):
    """lit_lens / dist_lens: the two codes' lengths by symbol.  hlit / hdist default to the last used symbol (257 / 1 at least), ops
    (the run-length coding of the hlit + hdist lengths) to rle_greedy's, cl_lens (the 19 code-length code lengths) to lengths_for of
    the ops' frequencies, hclen to the last non-zero of them in CL_ORDER.  With ops given, hlit / hdist only fill the header's fields."""
    return dict(type=2, final=final, tokens=list(tokens), lit_lens=list(lit_lens), dist_lens=list(dist_lens), hlit=hlit, hdist=hdist,
                hclen=hclen, cl_lens=cl_lens, ops=ops, eob=eob)


def raw_bits(pairs, final=False):
    """a "block" of bits as they are: [(value, count)] (BTYPE 3 and the like)"""
    return dict(type=3, final=final, pairs=list(pairs))


def token_freqs(tokens):
    """({literal/length symbol: count}, {distance symbol: count}) of the tokens, the end-of-block code included"""
    lf, df = {EOB: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            lf[t] = lf.get(t, 0) + 1
        elif isinstance(t[0], int):
            s = length_symbol(t[0], t[2] if len(t) > 2 else None)[0]
            d = dist_symbol(t[1])[0]
            lf[s] = lf.get(s, 0) + 1
            df[d] = df.get(d, 0) + 1
    return lf, df


def dyn_auto(tokens, final=False, **kw):
    """a dynamic block with Huffman lengths for the tokens' own frequencies (lengths_for); no distance used: HDIST 1 with an
    all-zero tree; one distance symbol used: that ONE code, of one bit -- RFC 1951's incomplete distance code"""
    lf, df = token_freqs(tokens)
    if len(lf) == 1:
        lf[0] = 1               # (a literal/length code needs a second symbol to be complete)
    ll = lengths_for(lf)
    lit = [ll.get(s, 0) for s in range(286)]
    if len(df) >= 2:
        dl = lengths_for(df)
        dist = [dl.get(s, 0) for s in range(30)]
    else:
        dist = [1 if s in df else 0 for s in range(30)]
    return dynamic(tokens, lit, dist, final, **kw)


class Stream:
    """one raw deflate stream: data, the text it stands for, starts = [(bit, text position)] of every block, marks, facts:
    max_lit_len / max_dist_len -- the longest code USED of either tree --, slow_symbols -- symbols used whose literal/length or
    distance code is longer than FAST bits --, longest_symbol -- most bits of one token, extra bits included"""

    def __init__(self):
        self.w = BitWriter()
        self.text = bytearray()
        self.starts = []
        self.types = []
        self.marks = {}
        self.facts = dict(max_lit_len=0, max_dist_len=0, slow_symbols=0, longest_symbol=0, blocks=0)
        self.headers = []       # of the dynamic blocks: (hlit, hdist, hclen, cl_lens, ops)

    @property
    def data(self):
        return self.w.getvalue()

    @property
    def bits(self):
        return self.w.pos

    def _tokens(self, tokens, lit, dist, eob):
        w, text, facts = self.w, self.text, self.facts
        for t in tokens:
            at = w.pos
            slow = False
            if isinstance(t, int):
                c, l = lit[t]
                w.bits(c, l)
                text.append(t)
                facts["max_lit_len"] = max(facts["max_lit_len"], l)
                slow = l > FAST
            elif isinstance(t[0], int):
                s, v, k = length_symbol(t[0], t[2] if len(t) > 2 else None)
                c, l = lit[s]
                w.bits(c, l)
                w.bits(v, k)
                ds, dv, dk = dist_symbol(t[1])
                dc, dl = dist[ds]
                w.bits(dc, dl)
                w.bits(dv, dk)
                facts["max_lit_len"] = max(facts["max_lit_len"], l)
                facts["max_dist_len"] = max(facts["max_dist_len"], dl)
                slow = l > FAST or dl > FAST
                if t[1] <= len(text):           # (a copy from before the text is what an invalid case is about: it makes no text)
                    for _ in range(t[0]):
                        text.append(text[-t[1]])
            elif t[0] == "mark":
                self.marks[t[1]] = (w.pos, len(text))
            elif t[0] == "litsym":
                w.bits(*lit[t[1]])
            elif t[0] == "distsym":
                s, v, k = length_symbol(t[1])
                w.bits(*lit[s])
                w.bits(v, k)
                w.bits(*dist[t[2]])
                w.bits(t[3], t[4])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                raise ValueError(t)
            facts["slow_symbols"] += slow
            facts["longest_symbol"] = max(facts["longest_symbol"], w.pos - at)
        if eob:
            w.bits(*lit[EOB])
            facts["max_lit_len"] = max(facts["max_lit_len"], lit[EOB][1])

    def add(self, block, final=None):
        """one block; final: overrides the block's own BFINAL"""
        w = self.w
        self.starts.append((w.pos, len(self.text)))
        self.types.append(block["type"])
        self.facts["blocks"] += 1
        w.bits(block["final"] if final is None else final, 1)
        w.bits(block["type"], 2)
        if block["type"] == 0:
            w.align(block["pad"])
            n = len(block["data"])
            w.bits(n, 16)
            w.bits(n ^ 0xFFFF if block["nlen"] is None else block["nlen"], 16)
            for c in block["data"]:
                w.bits(c, 8)
            self.text += block["data"]
        elif block["type"] == 1:
            self._tokens(block["tokens"], canonical(FIXED_LIT), canonical(FIXED_DIST), block["eob"])
        elif block["type"] == 2:
            lit_lens, dist_lens = block["lit_lens"], block["dist_lens"]
            hlit = block["hlit"] or max(257, max([i + 1 for i, l in enumerate(lit_lens) if l] or [0]))
            hdist = block["hdist"] or max(1, max([i + 1 for i, l in enumerate(dist_lens) if l] or [0]))
            ops = block["ops"]
            if ops is None:
                ops = rle_greedy((lit_lens + [0] * hlit)[:hlit] + (dist_lens + [0] * hdist)[:hdist])
            cl_lens = block["cl_lens"]
            if cl_lens is None:
                f = {}
                for op in ops:
                    s = op if isinstance(op, int) else op[0]
                    f[s] = f.get(s, 0) + 1
                if len(f) == 1:
                    f[(next(iter(f)) + 1) % 16] = 1
                d = lengths_for(f, 7)
                cl_lens = [d.get(s, 0) for s in range(19)]
            hclen = block["hclen"] or max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
            w.bits(hlit - 257, 5)
            w.bits(hdist - 1, 5)
            w.bits(hclen - 4, 4)
            for i in range(hclen):
                w.bits(cl_lens[CL_ORDER[i]], 3)
            cl = canonical(cl_lens)
            for op in ops:
                if isinstance(op, int):
                    w.bits(*cl[op])
                else:
                    w.bits(*cl[op[0]])
                    w.bits(op[1] - (3, 3, 11)[op[0] - 16], (2, 3, 7)[op[0] - 16])
            self.headers.append((hlit, hdist, hclen, list(cl_lens), list(ops)))
            self._tokens(block["tokens"], canonical(lit_lens), canonical(dist_lens), block["eob"])
        else:
            for v, k in block["pairs"]:
                w.bits(v, k)
        return self


def stream(blocks, final_last=True):
    """the blocks as one stream; final_last: BFINAL on the last block and on no other (None: as the blocks say)"""
    s = Stream()
    for i, b in enumerate(blocks):
        s.add(b, None if final_last is None else final_last and i + 1 == len(blocks))
    return s


# ---------------------------------------------------------------------------- containers
def gzip_member(data, text):
    """one gzip member around raw deflate data, CRC-32 and ISIZE those of the INTENDED text"""
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + data + zlib.crc32(text).to_bytes(4, "little") +
            (len(text) & 0xFFFFFFFF).to_bytes(4, "little"))


def bgzf_block(data, text):
    """one BGZF block: a gzip member with the 'BC' subfield (the member's size - 1), as tests/ingest_worker.bgzf writes them"""
    assert len(data) + 26 <= 65536 and len(text) <= 65536, (len(data), len(text))
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(data) + 25).to_bytes(2, "little") + data +
            zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little"))


BGZF_EOF = bgzf_block(b"\x03\x00", b"")


def bgzf_file(streams):
    """a BGZF file: one block per (data, text), then the EOF block"""
    return b"".join(bgzf_block(d, t) for d, t in streams) + BGZF_EOF


# ---------------------------------------------------------------------------- texts
def fasta(n, seed, name=None):
    """n bytes of FASTA-like text: a '>' line, then lines of 60 bases"""
    rng = random.Random(seed)
    out = bytearray(b">%s\n" % (name or b"s%d" % seed))
    while len(out) < n:
        out += bytes(rng.choices(b"ACGT", k=60)) + b"\n"
    return bytes(out[:n - 1] + b"\n")


def bases(n, seed):
    return bytes(random.Random(seed).choices(b"ACGT", k=n))


# ---------------------------------------------------------------------------- the case table
class Case:
    """name; valid (zlib's verdict, which test_deflate_craft.py checks); blocks; the stream made of them (stream(): data, text,
    starts, marks, facts); claims: {what the case is for: a check of the stream that must hold}, evaluated by the CPU test;
    bgzf: fits a BGZF block; degenerate: the literal/length tree is the end-of-block code alone (the strict-mode rule)"""

    def __init__(self, name, blocks, valid=True, claims=None, bgzf=True, degenerate=False):
        self.name, self.blocks, self.valid, self.claims, self.bgzf, self.degenerate = name, blocks, valid, claims or {}, bgzf, degenerate
        self._stream = None

    def stream(self):
        if self._stream is None:
            self._stream = stream(self.blocks)
        return self._stream

    @property
    def text(self):
        return bytes(self.stream().text)


CTRL = list(range(1, 9)) + list(range(14, 32))         # literals no text holds: the symbols complete_lens() may spend code space on
HEAD = b">x\n"


def _lits(b):
    return list(b)


LONG_RUN = 120


def _code_length_cases(add):
    text = HEAD + b"".join(bases(60, 7 + i) + b"\n" for i in range(4))
    # A, C, G, T, newline and the end-of-block code on 11 .. 15 bits: whole runs of symbols behind the decoders' 10-bit tables
    lit = complete_lens({ord("A"): 11, ord("C"): 12, ord("G"): 13, ord("T"): 14, 10: 15, EOB: 15, ord(">"): 9, ord("x"): 10}, 257, CTRL)
    add(Case("stair_literals", [dynamic(_lits(text), lit, [0])],
             claims={"every base and newline behind a table miss": lambda s: s.facts["slow_symbols"] >= len(text) - 2,
                     "EOB on 15 bits": lambda s: s.facts["max_lit_len"] == 15}))
    # the staircase itself: 1, 2, .., 15, 15 over sixteen symbols; the text's five on the long end
    order = CTRL[:10] + [ord("A"), ord("C"), ord("G"), ord("T"), 10, EOB]
    lens = [0] * 257
    for i, s in enumerate(order):
        lens[s] = min(i + 1, 15)
    body = b"".join(bases(60, 30 + i) + b"\n" for i in range(5))
    add(Case("staircase_1_to_15", [fixed(_lits(HEAD)), dynamic(_lits(body), lens, [0])],
             claims={"lengths 1, 2, .., 15, 15": lambda s: sorted(l for l in lens if l) == list(range(1, 16)) + [15],
                     "a run of table misses": lambda s: s.facts["slow_symbols"] == len(body)}))
    # distance codes of 11 .. 15 bits on the distances used
    dist = complete_lens({4: 11, 6: 12, 8: 13, 10: 14, 12: 15, 14: 15}, 30, [s for s in range(30)])
    toks = _lits(fasta(200, 11))
    for i, d in enumerate((5, 6, 9, 12, 17, 24, 33, 48, 65, 96, 129, 192) * 3):
        toks += [(3 + i, d)] + _lits(bases(1 + i % 5, 100 + i))
    lf, _ = token_freqs(toks)
    ll = lengths_for(lf)
    add(Case("long_distance_codes", [dynamic(toks, [ll.get(s, 0) for s in range(286)], dist)],
             claims={"distance codes up to 15 bits": lambda s: s.facts["max_dist_len"] == 15, "36 table misses": lambda s: s.facts["slow_symbols"] >= 36}))
    # the end-of-block code and a length symbol on 15 bits
    lit = complete_lens({ord("A"): 3, ord("C"): 3, ord("G"): 3, ord("T"): 3, 10: 3, ord(">"): 3, ord("x"): 3, 260: 15, EOB: 15}, 261, CTRL)
    toks = _lits(fasta(130, 12, b"x"))
    for i in range(12):
        toks += [(6, 20 + 7 * i)] + _lits(bases(i % 4, 200 + i))
    dl = lengths_for(token_freqs(toks)[1])
    add(Case("eob_and_length_on_15_bits", [dynamic(toks, lit, [dl.get(s, 0) for s in range(30)]),
                                            dynamic(_lits(b"ACGT\n"), lit, [0])],
             claims={"15-bit length codes": lambda s: s.facts["slow_symbols"] >= 12}))
    # the longest symbol there is: 15 + 5 + 15 + 13 bits, alone and in a run that crosses two 64-word windows of the input at
    # every byte offset the reader's word base can have (an 11-bit literal between two of them moves the phase by 59 bits)
    lit = complete_lens({ord("A"): 11, 281: 15, EOB: 15, 10: 2, ord("C"): 3, ord("G"): 3, ord("T"): 4}, 282, CTRL)
    dist = complete_lens({29: 15, 28: 15}, 30, list(range(28)))
    hist = fasta(24700, 13)
    toks = []
    for i in range(LONG_RUN):     # distances of symbol 29 (all-one extra bits: 32 768, once the text is that long) and of symbol 28
        d = (32768 if i >= 64 else 24577 + i) if i % 3 == 0 else 16385 + 97 * i
        toks += [("mark", "long%d" % i), (131 + (31 if i % 2 else i % 32), d), ("mark", "end%d" % i), ord("A")]
    toks += _lits(b"\n")

    def spans(s):
        return [(s.marks["long%d" % i][0], s.marks["end%d" % i][0]) for i in range(LONG_RUN)]
    # (48 bits: every one of them straddles a 32-bit word edge, wherever it starts)
    add(Case("longest_symbol", [stored(hist[:16384]), stored(hist[16384:]), dynamic(toks, lit, dist)],
             claims={"48 bits": lambda s: all(b - a == 48 for a, b in spans(s)) and s.facts["longest_symbol"] == 48,
                     "every start phase of a 64-bit window": lambda s: {a % 64 for a, _ in spans(s)} == set(range(64)),
                     "straddles two window swaps (word 63 -> 64, 127 -> 128) at every base offset": lambda s: all(
                         sum(1 for a, b in spans(s) if (a + 8 * k) // 2048 != (b - 1 + 8 * k) // 2048) >= 2 for k in range(4))}))


def _spelling_cases(add):
    hist = fasta(300, 21)
    toks = _lits(hist)
    for i in range(29):
        lo, hi = LEN_BASE[i], LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1
        for ln in sorted({lo, hi}):
            toks += [(ln, 1 + (7 * i + ln) % 250), ord("ACGT"[(i + ln) % 4])]
    toks += [(258, 61, "284+31"), 10, (258, 1, "284+31"), 10, (258, 64), 10]
    add(Case("all_length_codes_fixed", [fixed(toks)], claims={"258 both ways": lambda s: True}))
    lf, df = token_freqs(toks)
    ll, dl = lengths_for(lf), lengths_for(df)
    add(Case("all_length_codes_dynamic_hlit286", [dynamic(toks, [ll.get(s, 0) for s in range(286)], [dl.get(s, 0) for s in range(30)])],
             claims={"HLIT 286, 284 and 285 used": lambda s, ll=ll: s.headers[0][0] == 286 and ll[284] and ll[285]}))
    # all thirty distance codes, extra bits all zero and all one; distance 1 and 32 768 exactly (the latter reaches the text's first byte)
    hist = fasta(32768, 22)
    toks = [(9, 32768), 10]
    for i in range(30):
        lo, hi = DIST_BASE[i], DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1
        for d in sorted({lo, hi}):
            toks += [(3 + i % 9, d), ord("ACGT"[i % 4])]
    toks += [(258, 32768), 10, (4, 1), 10]
    add(Case("all_distance_codes_fixed", [stored(hist), fixed(toks)],
             claims={"distance 32 768 reaches byte 0": lambda s: s.text[32768:32777] == s.text[:9]}))
    lf, df = token_freqs(toks)
    ll, dl = lengths_for(lf), lengths_for(df)
    add(Case("all_distance_codes_dynamic_hdist30", [stored(hist[:16000]), stored(hist[16000:]), dynamic(toks, [ll.get(s, 0) for s in range(286)], [dl.get(s, 0) for s in range(30)])],
             claims={"HDIST 30": lambda s, dl=dl: s.headers[0][1] == 30 and all(dl.get(i) for i in range(30))}))


OVERLAP_DISTS = (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129)
OVERLAP_PHASES = (0, 1, 31, 62, 63)


def overlap_lengths(d):
    return sorted({n for n in (3, 4, d - 1, d, d + 1, 63, 64, 65, 2 * d + 1, 257, 258) if 3 <= n <= 258})


def _overlap_cases(add):
    """Every copy in a block of its own, behind `phase` literals: a block's end empties the decoders' output batch, so the copy
    starts with exactly `phase` bytes in it.  Two forms: fixed blocks (codes of <= 9 bits: the copy goes through the lanes' walk and,
    where its source lies inside the batch, through flush()'s pointer jumping) and dynamic blocks whose length symbols have 12-bit
    codes (the one-symbol path: place() and its o % dist)."""
    for d in OVERLAP_DISTS:
        lens = overlap_lengths(d)
        hist = fasta(192, 40 + d)
        wanted = {ord(c): 3 for c in "ACGT"}
        wanted.update({10: 4, ord(">"): 6, ord("s"): 6, EOB: 5})
        wanted.update({ord(c): 8 for c in "0123456789"})
        wanted.update({length_symbol(n)[0]: 12 for n in lens})
        lit = complete_lens(wanted, 286, CTRL)
        ds = dist_symbol(d)[0]
        dist = [0] * 30
        dist[ds] = dist[(ds + 1) % 30] = 1
        fx, dy, n = [fixed(_lits(hist))], [fixed(_lits(hist))], 0
        for ln in lens:
            for ph in OVERLAP_PHASES:
                toks = _lits(bases(ph, 1000 * d + 10 * ln + ph)) + [(ln, d)]
                fx.append(fixed(toks))
                dy.append(dynamic(toks, lit, dist))
                n += 1
        tail = _lits(b"\nACGT\n")
        fx.append(fixed(tail))
        dy.append(fixed(tail))
        add(Case("overlap_walk_d%d" % d, fx, claims={"copies": lambda s, n=n: s.facts["blocks"] == n + 2}))
        add(Case("overlap_place_d%d" % d, dy, claims={"every copy behind a table miss": lambda s, n=n: s.facts["slow_symbols"] == n}))


def _nl_block(p):
    """a dynamic block of p newlines on 1-bit codes: p + 1 bits behind a header of fixed size -- what moves a bit position by an odd amount"""
    lit = [0] * 257
    lit[10] = lit[EOB] = 1
    return dynamic([10] * p, lit, [0])


def _pad_to(s, want, mod):
    """empty fixed blocks (10 bits each) and newline blocks until the stream stands at bit `want` modulo `mod`"""
    for p in range(0, 4):
        head = [_nl_block(p)] if p else []
        bits = stream(head, None).bits
        for j in range(0, mod):
            if (s.w.pos + bits + 10 * j) % mod == want:
                return head + [fixed([])] * j
    raise AssertionError((want, mod))


def _bit_phase_cases(add):
    # a block start at every bit offset 0..31 of a word
    s, blocks, marked = Stream(), [], []
    for k in range(32):
        for b in _pad_to(s, k, 32) + [dyn_auto(_lits(fasta(70, 300 + k)))]:
            blocks.append(b)
            s.add(b, False)
        marked.append(len(blocks) - 1)
    blocks.append(fixed(_lits(b"ACGT\n")))
    add(Case("block_start_at_every_bit_of_a_word", blocks,
             claims={"32 offsets": lambda s: {s.starts[i][0] % 32 for i in marked} == set(range(32))}))
    # the final block's end-of-block code ending at each of the eight bit positions of a byte: bytes_used against the trailer
    for k in range(8):
        s, blocks = Stream(), [dyn_auto(_lits(fasta(90, 340 + k)))]
        s.add(blocks[0], False)
        last = fixed(_lits(b"ACGT\n"))
        bits_last = 3 + 8 * 5 + 7
        blocks += _pad_to(s, (k - bits_last) % 8, 8) + [last]
        add(Case("final_eob_ends_at_bit_%d" % k, blocks, claims={"ends there": lambda s, k=k: s.bits % 8 == k}))


def _block_structure_cases(add):
    t = [fasta(150, 400 + i) for i in range(8)]
    lit2 = [0] * 257
    lit2[10] = lit2[EOB] = 1
    empties = {"stored": stored(b""), "fixed": fixed([]), "dynamic": dynamic([], lit2, [0])}
    for name, e in empties.items():
        add(Case("run_of_empty_%s_blocks" % name, [dyn_auto(_lits(t[0]))] + [e] * 5 + [dyn_auto(_lits(t[1]))] + [e] * 3 + [fixed(_lits(t[2]))] + [e] * 2,
                 claims={"blocks": lambda s: s.facts["blocks"] == 13}))
        add(Case("final_empty_%s_block" % name, [dyn_auto(_lits(t[3])), dict(e)], claims={"final": lambda s: True}))
    # 200 consecutive blocks of one symbol each
    text = fasta(200, 410)
    blocks = []
    for i, c in enumerate(text):
        blocks.append(fixed([c]) if i % 3 == 0 else (stored(bytes([c]), pad=0x55) if i % 3 == 1 else dyn_auto([c])))
    add(Case("200_blocks_of_one_symbol", blocks, claims={"200": lambda s: s.facts["blocks"] == 200 and len(s.text) == 200}))
    # stored <-> Huffman with 0..7 pad bits in front of the stored block's LEN (the pad bits set: an inflater ignores them)
    s, blocks, pads = Stream(), [], []
    for k in range(8):
        head = dyn_auto(_lits(fasta(64 + k, 420 + k)))
        s.add(head, False)
        fill = _pad_to(s, (8 - k - 3) % 8, 8)
        for b in fill:
            s.add(b, False)
        st = stored(bases(50 + k, 430 + k) + b"\n", pad=0xFF)
        pads.append(-(s.w.pos + 3) % 8)
        s.add(st, False)
        blocks += [head] + fill + [st]
    add(Case("stored_behind_0_to_7_pad_bits", blocks + [fixed(_lits(b"ACGT\n"))], claims={"pads": lambda s: sorted(pads) == list(range(8))}))
    # a stored block arriving while the batch holds 1 byte and 63 bytes
    add(Case("stored_behind_partial_batches", [fixed(_lits(HEAD)), fixed([65]), stored(bases(100, 440) + b"\n"), fixed(_lits(bases(63, 441))),
                                               stored(bases(100, 442) + b"\n"), dyn_auto(_lits(bases(63, 443))), stored(b"\n" + bases(200, 444) + b"\n")]))
    # text_crc splits the text over the lanes from 8192 bytes on: one byte below, at, one above
    for n in (8191, 8192, 8193):
        body = fasta(n, 450 + n)
        add(Case("text_of_%d_bytes" % n, [stored(body[:4000]), dyn_auto(_lits(body[4000:6000])), fixed(_lits(body[6000:]))],
                 claims={"size": lambda s, n=n: len(s.text) == n}))
    # the largest stored block: a single member's only (a BGZF block holds 65 510 bytes of deflate data at most)
    add(Case("stored_65535", [fixed(_lits(HEAD)), stored(fasta(65535, 460)[3:] + b"ACG"), fixed(_lits(b"ACGT\n"))], bgzf=False,
             claims={"LEN 65535": lambda s: len(s.text) == 65535 + 3 + 5}))
    # what a piece decoded without its history meets at its very start: a copy from exactly 32 768 bytes in front of the block, one
    # from exactly 1 byte in front (a run: it starts in front of the block and goes on inside it), one that starts 10 bytes in
    # front and ends 10 bytes inside
    hist = fasta(32768, 470)
    add(Case("copies_at_the_edges_of_the_history", [stored(hist), dyn_auto([(9, 32768)] + _lits(bases(50, 471) + b"\n")),
                                                    dyn_auto([(5, 1)] + _lits(bases(55, 472) + b"\n")), fixed([(20, 10)] + _lits(bases(40, 473) + b"\n")),
                                                    dyn_auto([(258, 32768), (3, 1)] + _lits(b"\n"))],
             claims={"starts": lambda s: [at for _, at in s.starts] == [0, 32768, 32828, 32889, 32950]}))
    for name, b in (("stored", stored(t[4])), ("fixed", fixed(_lits(t[4]))), ("dynamic", dyn_auto(_lits(t[4])))):
        add(Case("final_%s_block" % name, [dyn_auto(_lits(t[5])), b]))
        add(Case("only_a_%s_block" % name, [b]))


def _header_cases(add):
    body = fasta(200, 500)
    lf, _ = token_freqs(_lits(body))
    auto_lit = [lengths_for(lf).get(s, 0) for s in range(257)]
    # HCLEN 5, the smallest a valid block can have (HCLEN 4 sends lengths for 16, 17, 18 and 0 only: every code length is zero and
    # there is no end-of-block code -- the invalid case hclen_4): symbols 1..256 on 8 bits each, all by code-length symbol 8
    lit = [0] + [8] * 256
    cl = [0] * 19
    cl[0] = cl[8] = 1
    add(Case("hclen_5", [dynamic(_lits(body), lit, [0], cl_lens=cl, ops=rle_plain(lit + [0]))],
             claims={"HCLEN 5": lambda s: s.headers[0][2] == 5}))
    # HCLEN 19 -- code-length symbol 15, the last of the order, has a code -- and a code-length code of 1, 2, .., 7, 7 bits whose
    # 7-bit codes are 15's and that of the rarest symbol the header uses
    text = b">\n" + b"".join(bases(60, 505 + i) + b"\n" for i in range(3))
    lit = [0] * 257
    for c, l in ((ord("A"), 2), (ord("C"), 2), (ord("G"), 2), (ord("T"), 3), (10, 4), (ord(">"), 5), (EOB, 5)):
        lit[c] = l
    ops = rle_greedy(lit + [0])
    f = {}
    for op in ops:
        u = op if isinstance(op, int) else op[0]
        f[u] = f.get(u, 0) + 1
    used = sorted(f, key=lambda u: (-f[u], u))
    assert len(used) == 7 and 15 not in used, used
    cl = [0] * 19
    for i, u in enumerate(used + [15]):
        cl[u] = min(i + 1, 7)
    add(Case("hclen_19_and_7_bit_code_length_codes", [dynamic(_lits(text), lit, [0], cl_lens=cl, ops=ops)],
             claims={"HCLEN 19": lambda s: s.headers[0][2] == 19,
                     "a 7-bit code is used": lambda s, u=used[6]: s.headers[0][3][u] == 7 and any((op if isinstance(op, int) else op[0]) == u for op in s.headers[0][4])}))
    # symbol 16 running from the literal/length lengths (257..259) into the distance lengths (0, 1); the last run -- zeros by 17 --
    # ends exactly at HLIT + HDIST
    text = b">x\n" + b"".join(bases(60, 515 + i) + b"\n" for i in range(3))
    lit = [0] * 260
    for c, l in ((ord("A"), 2), (ord("C"), 2), (ord("G"), 2), (ord("T"), 3), (10, 4), (ord(">"), 6), (ord("x"), 6), (256, 7), (257, 7), (258, 7), (259, 7)):
        lit[c] = l
    dist = [7, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0]
    ops = rle_greedy(lit[:256]) + [7, (16, 5), 6, 5, 4, 3, 2, 1, (17, 3)]
    toks = _lits(text) + [(3, 1), 10, (4, 2), (5, 3), 10, (3, 4), (4, 6), (5, 8), 10, (3, 12), (4, 16), 10]
    add(Case("repeat_16_runs_from_lengths_into_distances", [dynamic(toks, lit, dist, hlit=260, hdist=11, ops=ops)],
             claims={"the ops are the lengths": lambda s, want=lit + dist: rle_expand(s.headers[0][4]) == want,
                     "one 16 covers 257..259 and distances 0, 1": lambda s: (16, 5) in s.headers[0][4],
                     "the last run ends exactly at HLIT + HDIST": lambda s: s.headers[0][4][-1] == (17, 3)}))
    # symbol 16 directly behind 17 and behind 18 (it repeats ZERO), symbol 18 with 138, HLIT 286
    text = b">s\n" + b"".join(bases(60, 510 + i) + b"\n" for i in range(3))
    lit = complete_lens({ord(">"): 4, ord("s"): 4, 10: 3, ord("A"): 3, ord("C"): 3, ord("G"): 3, ord("T"): 2, EOB: 5, 283: 5, 284: 5, 285: 5}, 286, [])
    want = lit + [1, 1]
    ops, i, first17, first18 = [], 0, True, True
    while i < len(want):
        if want[i]:
            ops.append(want[i])
            i += 1
            continue
        j = i
        while j < len(want) and not want[j]:
            j += 1
        run = j - i
        if run >= 138:
            ops.append((18, 138))
            run -= 138
        elif run >= 14 and first18:
            ops += [(18, 11), (16, 3)]
            run -= 14
            first18 = False
        elif run >= 6 and first17:
            ops += [(17, 3), (16, 3)]
            run -= 6
            first17 = False
        ops += rle_greedy([0] * run)
        i = j
    toks = _lits(text) + [(258, 2), 10, (258, 1, "284+31"), 10, (227, 2), 10]

    def behind(ops, x):
        return any(a == x and b == (16, 3) for a, b in zip(ops, ops[1:]))
    add(Case("repeat_16_behind_17_and_18_and_18_with_138", [dynamic(toks, lit, [1, 1], hlit=286, hdist=2, ops=ops)],
             claims={"the ops are the lengths": lambda s, want=want: rle_expand(s.headers[0][4]) == want,
                     "16 behind 17 and behind 18": lambda s: behind(s.headers[0][4], (17, 3)) and behind(s.headers[0][4], (18, 11)),
                     "18 with 138": lambda s: (18, 138) in s.headers[0][4]}))
    # HDIST 1, its one code of one bit used; an all-zero distance tree under literals only; the one code of one bit at a higher symbol
    toks = _lits(body) + [(20, 1), 10]
    l2 = lengths_for(token_freqs(toks)[0])
    add(Case("hdist_1_one_code_of_one_bit_used", [dynamic(toks, [l2.get(s, 0) for s in range(286)], [1])],
             claims={"HDIST 1": lambda s: s.headers[0][1] == 1}))
    add(Case("all_zero_distance_tree", [dynamic(_lits(body), auto_lit, [0])], claims={"HDIST 1": lambda s: s.headers[0][1] == 1}))
    toks = _lits(body) + [(20, 40), 10, (3, 33), 10, (258, 48), 10]
    l2 = lengths_for(token_freqs(toks)[0])
    add(Case("one_distance_code_of_one_bit_at_symbol_10", [dynamic(toks, [l2.get(s, 0) for s in range(286)], [0] * 10 + [1])],
             claims={"HDIST 11": lambda s: s.headers[0][1] == 11}))
    # the degenerate literal/length tree: the end-of-block code alone, on ONE bit (zlib takes it: an empty block)
    lit = [0] * 257
    lit[EOB] = 1
    add(Case("eob_alone_on_one_bit", [dyn_auto(_lits(body)), dynamic([], lit, [0]), fixed(_lits(b"ACGT\n"))], degenerate=True,
             claims={"three blocks": lambda s: s.facts["blocks"] == 3}))


def _invalid_cases(add):
    body = fasta(120, 600)
    toks = _lits(body)
    lf, _ = token_freqs(toks + [(10, 20)])
    ll = lengths_for(lf)
    lit = [ll.get(s, 0) for s in range(286)]
    # (the good block in front of the fault has a complete distance code of two symbols, so that nothing but the fault is unusual)
    gl = lengths_for(token_freqs(_lits(fasta(100, 601)))[0])
    good = dynamic(_lits(fasta(100, 601)), [gl.get(s, 0) for s in range(257)], [1, 1])

    def bad(name, blocks, **kw):
        add(Case("invalid_" + name, blocks, valid=False, **kw))
    bad("one_distance_code_of_two_bits_used", [good, dynamic(toks + [(10, 20)], lit, [0] * 8 + [2])])
    over = list(lit)
    over[ord("N")] = 1
    bad("oversubscribed_literal_tree", [good, dynamic(toks, over, [0])])
    bad("oversubscribed_distance_tree", [good, dynamic(toks + [(10, 20)], lit, [1, 1, 0, 0, 0, 0, 0, 0, 1])])
    two = [0] * 257
    two[10], two[EOB] = 2, 2
    bad("incomplete_literal_tree_of_two_codes", [good, dynamic([10, 10], two, [0])])
    cl = [0] * 19
    cl[16] = cl[0] = cl[8] = 2
    cl[7] = 2
    bad("repeat_16_as_the_first_length", [good, dynamic([], [0] + [8] * 256, [0], hlit=257, hdist=1, cl_lens=cl, ops=[(16, 3)] + [8] * 254 + [0])])
    cl = [0] * 19
    cl[0] = cl[8] = 2
    cl[18] = 1
    bad("run_beyond_hlit_plus_hdist", [good, dynamic([], [0] + [8] * 256, [0], hlit=257, hdist=1, cl_lens=cl, ops=[0] + [8] * 256 + [(18, 11)])])
    noeob = [0] * 257
    for s in range(256):
        noeob[s] = 8
    bad("no_end_of_block_code", [good, dynamic(_lits(b"ACGT\n"), noeob, [0], eob=False)])
    cl = [0] * 19
    cl[16], cl[17], cl[18], cl[0] = 2, 2, 2, 2
    bad("hclen_4", [good, dynamic([], [0] * 257, [0], hlit=257, hdist=1, hclen=4, cl_lens=cl, ops=[(18, 138), (18, 120)], eob=False)])
    bad("btype_3", [good, raw_bits([(0x2AAAA, 20)])])
    bad("stored_nlen_wrong", [good, stored(b"ACGT\n", nlen=0x1234)])
    bad("distance_before_the_text", [dyn_auto(_lits(body[:60]) + [(10, 61)] + _lits(body[60:]))])
    bad("distance_one_before_the_text", [fixed([(3, 1)] + toks)])
    bad("literal_length_symbol_286_in_a_fixed_block", [good, fixed(toks + [("litsym", 286)] + toks)])
    bad("distance_symbol_30_in_a_fixed_block", [good, fixed(toks + [("distsym", 5, 30, 0, 0)] + toks)])
    one = dynamic(toks + [(10, 20), ("litsym", 257 + 7), ("bits", 1, 1)] + toks, lit, [0] * 8 + [1])
    bad("missing_code_of_a_one_code_distance_tree", [good, one])
    bad("hlit_287", [good, dynamic(toks, lit + [0], [0], hlit=287, hdist=1, ops=rle_greedy(lit + [0] + [0]))])
    bad("hdist_31", [good, dynamic(toks, lit, [0] * 31, hlit=286, hdist=31, ops=rle_greedy(lit + [0] * 31))])
    # data that ends before the end-of-block code: the stream simply stops (in a container the trailer follows at once)
    bad("ends_before_end_of_block", [good, dynamic(toks, lit, [0], eob=False)], claims={"truncated": lambda s: True})


_CASES = None


def cases():
    """the table: [Case], built once per process"""
    global _CASES
    if _CASES is None:
        out = []
        for part in (_code_length_cases, _spelling_cases, _overlap_cases, _bit_phase_cases, _block_structure_cases, _header_cases, _invalid_cases):
            part(out.append)
        assert len({c.name for c in out}) == len(out)
        _CASES = out
    return _CASES


def valid_cases():
    return [c for c in cases() if c.valid]


def invalid_cases():
    return [c for c in cases() if not c.valid]


# ---------------------------------------------------------------------------- members made of many cases
def member_text_block(s, n, seed):
    """a dynamic block of ~n bytes of FASTA-like text behind what Stream s already holds: literals, and copies that reach back
    up to 32 768 bytes into it -- into the blocks of other cases too"""
    body, toks, i, rng = fasta(n, seed), [], 0, random.Random(seed)
    have = len(s.text)
    while i < n:
        if have + i > 400 and rng.random() < 0.02:
            toks.append((rng.randrange(3, 40), rng.randrange(1, min(have + i, 32768) + 1)))
            i += toks[-1][0]
        else:
            toks.append(body[i])
            i += 1
    return dyn_auto(toks)


def concat_member(parts, seed, text_bytes=3000, texts_between=3):
    """ONE raw deflate stream made of several cases' blocks (parts: lists of blocks), `texts_between` dynamic text blocks in front
    of each -- three in a row is what the host's block finder demands of a starting point -- and behind the last, then a final
    fixed block.  A case's own copies stay inside its own text.  -> Stream"""
    s, k = Stream(), 0
    for blocks in list(parts) + [[]]:
        for _ in range(texts_between):
            s.add(member_text_block(s, text_bytes, seed + k), False)
            k += 1
        for b in blocks:
            s.add(b, False)
    s.add(fixed(_lits(b"ACGT\n")), True)
    return s
