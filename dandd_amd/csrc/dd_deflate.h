// dd_deflate.h -- what the device inflate's two files share (device code): the wave's LDS layout of a deflate block's code
// tables, the bit reader, the table builders, the one-symbol literal/length decoder and the text's CRC-32.  dd_ginflate.hip holds the decoder
// (inflate_kernel), dd_gunzip.hip the pipeline that cuts a single-member gzip file into pieces for it (its block-start finder
// tries headers and first symbols with the decoder's own tables).  Everything here has internal linkage: both files include it.
#pragma once
#include "dd_common.h"

namespace dd {
namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// (round 5, measured and put back: 9-bit tables -- 2 KiB each, 5.25 KiB per wave instead of 9.25, 24-28 waves per CU instead of
// 17 -- gave ten gzip -1 files 8.0 -> 8.3 Gbp/s and took one 400 Mbp gzip -6 file from 10.3 to 9.4 (codes of 10 bits go through
// decode_slow); BGZF and gzip -6 directories unchanged: profiles/r05_gunzip.txt)
constexpr int FAST = 10;
constexpr uint32_t kTableBytes = 4u << FAST;
constexpr uint32_t kLitInfo = 0;                  // u32[1 << FAST]: literal / length code table (FAST-bit lookup)
constexpr uint32_t kDistInfo = kLitInfo + kTableBytes;  // u32[1 << FAST]: distance code table
constexpr uint32_t kLitCount = kDistInfo + kTableBytes; // u16[16] + u16[288]: codes longer than FAST bits, puff-style
constexpr uint32_t kLitSymbol = kLitCount + 32u;
constexpr uint32_t kDistCount = kLitSymbol + 576u;
constexpr uint32_t kDistSymbol = kDistCount + 32u;
constexpr uint32_t kLens = kDistSymbol + 64u;     // u8[320]: code lengths while a table is built
constexpr uint32_t kClInfo = kLens + 320u;        // u16[128]: code-length code table (7-bit lookup)
constexpr uint32_t kInflateLds = (kClInfo + 256u + 15u) & ~15u;   // 9.25 KiB: seventeen one-wave workgroups per CU
static_assert(kTableBytes >= 1024u, "text_crc keeps its 256-entry table in the literal table's place");

__constant__ uint16_t c_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ constexpr uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // (constexpr: the finder's unrolled loops compare its entries at compile time)

DD_D uint32_t& l32(uint32_t off) { return *reinterpret_cast<uint32_t*>(g_lds + off); }
DD_D uint16_t& l16(uint32_t off) { return *reinterpret_cast<uint16_t*>(g_lds + off); }
DD_D uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
DD_D uint64_t uni64(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }
DD_D uint32_t gload1(const uint8_t* p) { return *(const DD_GLOBAL uint8_t*)p; }
DD_D uint32_t lane_value(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
DD_D uint32_t bperm(uint32_t lane_index, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lane_index << 2), (int)v); }

// The wave's bit reader: every lane holds the same state.  The block's compressed words come through the lanes
// themselves: lane j keeps word (window + j) of the input, a refill of the bit buffer is ONE v_readlane, and the next
// window of 256 bytes is asked for (one coalesced load) when the current one is entered, a whole window ahead of need.
// (Words taken from HBM as they were needed cost a memory round trip per 32 bits of input: 6.5 ms per block; a ring in
// LDS costs eight instructions per word and 2 KiB per wave; profiles/r04_bgzf.txt.)
struct WBits {
    const uint32_t* w;     // the input as 4-byte aligned words
    uint32_t wi;           // next word to put into `ahead`
    uint32_t nwords;       // words that belong to the block (beyond: zeros)
    uint32_t cur, nxt;     // this lane's word of the window that holds word wi, and of the one after it
    uint64_t buf;
    int cnt;
    uint32_t ahead;        // W[wi - 1], already taken from the window
    DD_D uint32_t fetch(uint32_t first) const {   // this lane's word of the 64 that start at `first`
        const uint32_t i = first + (threadIdx.x & 63u);
        return i < nwords ? gload4(w + i) : 0u;
    }
    DD_D uint32_t word() {   // W[wi++]
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(wi & 63u));
        ++wi;
        if ((wi & 63u) == 0u) {
            cur = nxt;
            nxt = fetch(wi + 64u);
        }
        return v;
    }
    DD_D void seek(uint32_t q) {   // the next word() is W[q]
        wi = q;
        cur = fetch(q & ~63u);
        nxt = fetch((q & ~63u) + 64u);
    }
    DD_D void start_at(uint32_t q, uint32_t r) {   // the reader stands at bit r (< 32) of W[q]
        seek(q);
        buf = word();
        ahead = word();
        buf >>= r;
        cnt = 32 - (int)r;
        refill();
    }
    DD_D void init(const uint8_t* p, uint32_t nbytes) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const uint32_t skip = (uint32_t)(a & 3u);
        w = reinterpret_cast<const uint32_t*>(a - skip);
        nwords = (skip + nbytes + 3u) / 4u;
        start_at(0, 8u * skip);
    }
    DD_D uint64_t bit_pos() const { return (uint64_t)(wi - 1u) * 32u - (uint64_t)cnt; }   // bits of W consumed (`ahead` is read but not in the buffer)
    DD_D void refill() {   // from >= 0 valid bits to >= 32
        buf |= (uint64_t)ahead << cnt;
        cnt += 32;
        ahead = word();
    }
    DD_D void need() { if (cnt <= 32) refill(); }   // more than 32 valid bits afterwards
    DD_D uint32_t peek(int k) const { return (uint32_t)buf & ((1u << k) - 1u); }   // k <= 16
    DD_D void drop(int k) { buf >>= k; cnt -= k; }
    DD_D uint32_t take(int k) {
        if (cnt < k) refill();
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    // bytes of the input consumed so far, counting a partly used byte as consumed
    DD_D uint32_t bytes_used(const uint8_t* p) const {
        return (uint32_t)((bit_pos() + 7ull) / 8ull - (reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(w)));
    }
};

// A canonical Huffman code from the lengths at g_lds[kLens + first .. + n): info table (FAST-bit lookup) at `info`, the
// puff-style count / symbol arrays at `cnt_off` / `sym_off` for longer codes.  kind: 0 literal/length tree, 1 distance tree.
// Wave-uniform; returns false when the lengths are not a usable code.
__device__ __noinline__ bool build_table(uint32_t first, int n, int kind, uint32_t info, uint32_t cnt_off, uint32_t sym_off) {
    const uint32_t lane = threadIdx.x & 63u;
    // count[l]: lanes 0..15 hold one length each
    uint32_t mine = 0;
    if (lane < 16u)
        for (int i = 0; i < n; ++i) mine += (g_lds[kLens + first + i] == lane) ? 1u : 0u;
    if (lane < 16u) l16(cnt_off + 2u * lane) = (uint16_t)mine;
    for (uint32_t i = lane; i < (1u << FAST); i += 64u) l32(info + 4u * i) = 0;
    __builtin_amdgcn_wave_barrier();
    int left = 1, nonzero = 0;
    // next canonical code and next index into symbol[] of each length: lane l keeps length l's pair
    uint32_t my_code = 0, my_off = 0;
    uint32_t c = 0, o = 0;
    for (uint32_t l = 1; l <= 15u; ++l) {
        const uint32_t cl = uni(l16(cnt_off + 2u * l));
        left = (left << 1) - (int)cl;
        if (left < 0) return false;
        nonzero += (int)cl;
        if (lane == l) my_code = c, my_off = o;
        c = (c + cl) << 1;
        o += cl;
    }
    if (nonzero == 0) return kind == 1;   // (a block of literals only may come with no distance code at all: RFC 1951, 3.2.7)
    // incomplete: only ONE code of ONE bit may be, as in zlib's inflate_table (a used distance code of two bits and more with no
    // sibling is refused there, and was sketched here); the literal/length tree of an empty block may be the end-of-block code alone
    if (left > 0 && !(nonzero == 1 && uni(l16(cnt_off + 2u)) == 1u)) return false;
    // every symbol in turn (uniform), its table replicas spread over the lanes
    for (int i = 0; i < n; ++i) {
        const uint32_t l = uni((uint32_t)g_lds[kLens + first + i]);
        if (!l) continue;
        const uint32_t cd = lane_value(my_code, l), at = lane_value(my_off, l);
        if (lane == l) ++my_code, ++my_off;
        if (lane == 0) l16(sym_off + 2u * at) = (uint16_t)i;
        if (l > (uint32_t)FAST) continue;
        uint32_t v;
        if (kind == 0) {
            if (i < 256) v = l | (1u << 4) | ((uint32_t)i << 11);
            else if (i == 256) v = l | (2u << 4);
            else if (i <= 285) v = l | (3u << 4) | ((uint32_t)c_len_extra[i - 257] << 7) | ((uint32_t)c_len_base[i - 257] << 11);
            else v = 0;   // 286, 287: never valid in a stream
        } else {
            v = i <= 29 ? (l | (3u << 4) | ((uint32_t)c_dist_extra[i] << 7) | ((uint32_t)c_dist_base[i] << 11)) : 0u;
        }
        const uint32_t rev = __builtin_bitreverse32(cd) >> (32u - l);
        for (uint32_t f = rev + (lane << l); f < (1u << FAST); f += 64u << l) l32(info + 4u * f) = v;
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// a code longer than FAST bits (or an invalid one), from the low bits of `bits`: walk the lengths, one bit at a time.
// -> symbol << 4 | code length, or ~0u when there is no such code.  (The bit reader stays in the caller's registers:
// handing it over by reference put it, and with it every shift of the hot loop, into scratch memory.)
__device__ __noinline__ uint32_t decode_slow(uint64_t bits, uint32_t cnt_off, uint32_t sym_off) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bits & 1ull);
        bits >>= 1;
        const int c = (int)uni(l16(cnt_off + 2u * (uint32_t)l));
        if (code - c < first) return (uni(l16(sym_off + 2u * (uint32_t)(index + (code - first)))) << 4) | (uint32_t)l;
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return ~0u;
}

// ---- CRC-32 of the inflated text (the member's trailer carries it) ----
// x^(2^n) mod P for n = 0..31 in zlib's reflected notation (bit 31 = x^0), P = 0xedb88320: each entry is the square of
// the one before (multmodp below); generated by squaring 0x40000000 (= x^1).
__constant__ uint32_t c_x2n[32] = {0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu, 0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu, 0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu, 0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};

// a(x) * b(x) mod P.  `a` is wave-uniform (the loop's exit is), b is per lane.
DD_D uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u;; m >>= 1) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1u)) == 0u) break;
        }
        b = (b >> 1) ^ ((b & 1u) ? 0xedb88320u : 0u);
    }
    return p;
}

// The CRC-32 of text[0, n), by the whole wave: lane i takes the i-th 1/64 of the text (the FIRST lane's part is the short
// one, so that every right-hand operand of a combination has a length that depends on the level only), byte-wise with a
// 256-entry table in LDS -- the Huffman tables' place, the block is decoded --, then six levels of
//   crc(A || B) = crc(A) * x^(8 |B|) mod P  ^  crc(B)          (zlib's crc32_combine).
// ~1 % of a block's instructions.  The text is read back past the vector L1; the caller has waited for its stores.
__device__ __noinline__ uint32_t text_crc(const uint8_t* text, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = lane; i < 256u; i += 64u) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xedb88320u : 0u);
        l32(kLitInfo + 4u * i) = c;
    }
    __builtin_amdgcn_wave_barrier();
    auto byte_in = [](uint32_t crc, uint32_t v) { return l32(kLitInfo + 4u * ((crc ^ v) & 255u)) ^ (crc >> 8); };
    uint32_t lo = 0, hi = n, len = 0;
    if (n >= 8192u) {   // (shorter: a file's last block; every lane does all of it)
        len = (n + 63u) / 64u;
        const uint32_t pad = 64u * len - n;   // < 64 <= len
        lo = lane ? lane * len - pad : 0u;
        hi = (lane + 1u) * len - pad;
    }
    uint32_t crc = ~0u, p = lo;
    for (; p < hi && ((reinterpret_cast<uintptr_t>(text) + p) & 3u); ++p) crc = byte_in(crc, gload1_fresh(text + p));
    for (; p + 4u <= hi; p += 4u) {
        const uint32_t v = gload4_fresh(text + p);
        crc = byte_in(crc, v);
        crc = byte_in(crc, v >> 8);
        crc = byte_in(crc, v >> 16);
        crc = byte_in(crc, v >> 24);
    }
    for (; p < hi; ++p) crc = byte_in(crc, gload1_fresh(text + p));
    crc = ~crc;
    if (n >= 8192u) {
        uint32_t c = 0x80000000u;   // x^(8 len): x^0, times x^(2^(k + 3)) for every bit k of len
        for (uint32_t k = 0, m = len; m; m >>= 1, ++k)
            if (m & 1u) c = uni(multmodp(uni(c_x2n[(k + 3u) & 31u]), c));
        for (int j = 0; j < 6; ++j) {
            const uint32_t right = (uint32_t)__shfl_down((int)crc, 1u << j);
            crc = multmodp(c, crc) ^ right;
            c = uni(multmodp(c, c));
        }
    }
    return uni(crc);
}

// The header of a dynamic-Huffman block (the reader stands behind BTYPE): code-length code, the two trees' code lengths,
// both symbol tables into LDS.  Wave-uniform; false: not a valid header.
DD_D bool dynamic_tables(WBits& b) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t hlit = b.take(5) + 257u, hdist = b.take(5) + 1u, hclen = b.take(4) + 4u;
    if (hlit > 286u || hdist > 30u) return false;
    // the code-length code: 19 lengths of 3 bits, a 7-bit table
    if (lane < 19u) g_lds[kLens + lane] = 0;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t v = b.take(3);
        if (lane == 0) g_lds[kLens + c_cl_order[i]] = (uint8_t)v;
    }
    __builtin_amdgcn_wave_barrier();
    {
        int left = 1;
        uint32_t mine = 0;   // lane l: how many of the 19 have length l, then its next code
        if (lane < 8u)
            for (int i = 0; i < 19; ++i) mine += ((uint32_t)g_lds[kLens + i] == lane) ? 1u : 0u;
        const uint32_t zeros = lane_value(mine, 0);
        uint32_t c = 0, my_code = 0;
        for (uint32_t l = 1; l <= 7u; ++l) {
            const uint32_t cl = lane_value(mine, l);
            left = (left << 1) - (int)cl;
            if (lane == l) my_code = c;
            c = (c + cl) << 1;
        }
        if (left != 0 && !(zeros == 18u && left > 0)) return false;   // (one code of one bit is tolerated, as zlib does)
        for (uint32_t i = lane; i < 128u; i += 64u) l16(kClInfo + 2u * i) = 0;
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < 19; ++i) {
            const uint32_t l = uni((uint32_t)g_lds[kLens + i]);
            if (!l) continue;
            const uint32_t cd = lane_value(my_code, l);
            if (lane == l) ++my_code;
            const uint32_t rev = __builtin_bitreverse32(cd) >> (32u - l);
            for (uint32_t f = rev + (lane << l); f < 128u; f += 64u << l) l16(kClInfo + 2u * f) = (uint16_t)(l | ((uint32_t)i << 4));
        }
        __builtin_amdgcn_wave_barrier();
    }
    // the literal/length and distance code lengths, run-length coded
    uint32_t i = 0, prev = 0;
    while (i < hlit + hdist) {
        b.need();
        const uint32_t e = uni(l16(kClInfo + 2u * b.peek(7)));
        if (!e) return false;
        b.drop((int)(e & 15u));
        const uint32_t s = e >> 4;
        uint32_t rep = 1, val = s;
        if (s == 16u) {
            if (!i) return false;
            val = prev;
            rep = 3u + b.take(2);
        } else if (s == 17u) {
            val = 0;
            rep = 3u + b.take(3);
        } else if (s == 18u) {
            val = 0;
            rep = 11u + b.take(7);
        }
        if (i + rep > hlit + hdist) return false;
        // (lengths of the two trees go to their own places: literal/length at 0.., distance at 288..)
        for (uint32_t r = lane; r < rep; r += 64u) {
            const uint32_t sym = i + r;
            g_lds[kLens + (sym < hlit ? sym : 288u + (sym - hlit))] = (uint8_t)val;
        }
        i += rep;
        prev = val;
    }
    __builtin_amdgcn_wave_barrier();
    if (uni((uint32_t)g_lds[kLens + 256u]) == 0u) return false;   // no end-of-block code
    if (!uni(build_table(0, (int)hlit, 0, kLitInfo, kLitCount, kLitSymbol)) || !uni(build_table(288, (int)hdist, 1, kDistInfo, kDistCount, kDistSymbol))) return false;
    return true;
}

// ---- one literal/length symbol from the low bits of `bits` (64 of them, handed over BY VALUE: see decode_slow), with the block's
// tables: the table's entry, or decode_slow for a code longer than FAST bits.  Wave-uniform.  The callers (the one-symbol path of
// inflate_kernel, the trial decoding of find_starts_kernel) drop `len` bits, then the `extra` ones.  kind: 1 a literal (base: the
// byte), 2 end of block, 3 a match (base + extra bits: its length), 0 no such code; len: the code's bits.
// (The distance code behind a length is decoded at the two sites themselves: a dist_code beside this one made the compiler
// change inflate_kernel<3>'s window loop -- profiles/kinflate_shared_decoder.txt.)
struct LitLenCode { uint32_t kind, extra, base, len; };
DD_D LitLenCode litlen_code(uint64_t bits) {
    const uint32_t e = uni(l32(kLitInfo + 4u * ((uint32_t)bits & ((1u << FAST) - 1u))));
    if (e) return {(e >> 4) & 7u, (e >> 7) & 15u, e >> 11, e & 15u};
    const uint32_t rs = uni(decode_slow(bits, kLitCount, kLitSymbol));   // a code longer than the table's 10 bits
    const uint32_t sy = rs >> 4;
    if (rs == ~0u || sy > 285u) return {0u, 0u, 0u, 0u};   // (286, 287: never valid in a stream)
    return {sy < 256u ? 1u : (sy == 256u ? 2u : 3u), sy > 256u ? uni((uint32_t)c_len_extra[sy - 257u]) : 0u,
            sy < 256u ? sy : (sy > 256u ? uni((uint32_t)c_len_base[sy - 257u]) : 0u), rs & 15u};
}

// The 32 bits from bit t (< 96) on of the words a, b, c, d: t's word picks the pair, v_alignbit shifts it.  A lane's window of
// 64 (96) bits is two (three) of these over five (six) consecutive words; the selects they share are computed once.
DD_D uint32_t window32(uint32_t t, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t kq = t >> 5, lo = kq == 0u ? a : (kq == 1u ? b : c), hi = kq == 0u ? b : (kq == 1u ? c : d);
    return __builtin_amdgcn_alignbit(hi, lo, t & 31u);
}

// Which file of a batch does entry `idx` of a batch-wide table (pieces, groups, 64 KiB chunks) belong to?  first(f): the first
// entry of file f -- read the way the caller needs it (uni() in a one-wave kernel).  A batch holds a few files: a linear walk.
template <typename First>
DD_D int file_of(int nfiles, uint32_t idx, First first) {
    int f = 0;
    while (f + 1 < nfiles && idx >= first(f + 1)) ++f;
    return f;
}

}  // namespace
}  // namespace dd
