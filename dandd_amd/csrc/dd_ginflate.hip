// dd_ginflate.hip -- gzip inflated on the GPU, straight into the FASTA buffer K0 reads: BGZF blocks, and ordinary .gz files.
//
// Real genome directories hold .fa.gz (/root/reference/lib/species_specifics.py:93) and every `dashing sketch` job of
// the reference inflates its input again (lib/huffman_dandd.py:214-218: one process per k).  On the host ten 50 Mbp
// .gz files at once are bound by the CPUs' aggregate inflate rate (3.8-5.6 Gbp/s on 16 cores, profiles/r03_ingest_gzip.txt)
// while the kernels behind them run at 20-36 Gbp/s.  A BGZF file (bgzip, htslib) is a sequence of independent gzip
// members of <= 64 KiB of text each, every one saying its own compressed size: they can be decoded anywhere, in any order.
//
// One wave per block.  A deflate stream is a serial thing -- every Huffman code starts where the previous one ended --,
// but the wave does not walk it one symbol at a time: LANE i DECODES THE SYMBOL THAT WOULD START AT BIT i of a 64-bit
// window (literal/length code, extra bits, distance code, extra bits: two table gathers from LDS), a walk follows the
// chain of symbols that really are there (round 4: scalar, one v_readlane each; round 5: by all lanes at once, pointer
// jumping -- parallel_walk), and the lanes of the 64-byte output batch look up the symbol they belong to and note where
// their byte comes from -- a literal, or an earlier position of the text, which may lie inside the batch itself (resolved
// by pointer jumping when the batch leaves, round 5).  A batch costs ONE load and ONE contiguous store.  Block headers,
// code tables (built code by code, the replicas of a code spread over the lanes), codes longer than the tables' 10 bits
// and copies that do not fit what is left of a batch go one symbol at a time.
// The block's TEXT lives where it is going -- the FASTA buffer in HBM --, not in LDS: a wave needs 9.25 KiB of LDS (its
// code tables), seventeen waves share a CU, and the serial chain of one block hides behind sixteen others.  What bounds a
// launch is the CU's scalar issue slot: instructions per symbol (profiles/r04_bgzf.txt: 10 ms per block -> 3.1).
// A copy reads what earlier batches of the same wave stored: a batch waits for the stores before it (issued a batch ago:
// free) and reads past the vector L1 (sc1).
// Anything that is not a valid block -- bad code lengths, a distance before the block's start, a length that does not
// match the member's ISIZE, a text whose CRC-32 is not the member's (the wave reads its text back: text_crc) -- raises the
// launch's error count and the caller runs the call again with the host decoder (dd_inflate.h), which words the error.
//
// ORDINARY .gz files (ONE gzip member) are cut into pieces by dd_gunzip.hip (launch_gunzip_members), which has the same
// decoder decode each piece WITHOUT the 32 KiB in front of it (inflate_kernel<3>, <1>, <2>: launch_inflate_pieces).
// What the two files share -- bit reader, code tables, the one-symbol literal/length decoder, the text's CRC-32 -- is dd_deflate.h.
#include "dd_common.h"
#include "dd_deflate.h"
#include "dd_kernels.h"

namespace dd {

// the piece a wave of the raw-deflate modes works on: entry `idx` of the batch's piece table
struct PieceRef {
    int file;
    uint64_t start, end;   // bit positions (a 3 Gbp assembly's .gz has 7 x 10^9); end = ~0: up to the stream's final block
    uint32_t j, ranges;    // the finder range it starts in, and how many ranges it runs over
};
DD_D bool piece_of(const RawFile* files, int nfiles, const uint64_t* starts, uint32_t idx, PieceRef& r) {
    const int f = file_of(nfiles, idx, [&](int i) { return uni(files[i].piece0); });
    const uint32_t j = idx - uni(files[f].piece0), ng = uni(files[f].nguess);
    r.file = f;
    r.start = uni64(starts[idx]);
    r.end = ~0ull;
    r.j = j;
    r.ranges = ng - j;
    if (j >= ng || r.start == ~0ull) return false;
    for (uint32_t k = j + 1; k < ng; ++k) {
        const uint64_t e = uni64(starts[idx - j + k]);
        if (e != ~0ull) {
            r.end = e;
            r.ranges = k - j;
            break;
        }
    }
    return true;
}

// ---- the walk over a window's symbols, all lanes at once (round 5) ------------------------------------------------------
// The scalar walk below follows the chain of symbols one v_readlane and ~20 scalar instructions at a time.  That is the right
// shape for gzip -6 text -- three or four matches per 64-bit window -- and the wrong one for gzip -1 and for anything else
// that is mostly LITERALS: DNA's four letters get 2-bit codes, a window holds up to 32 symbols, and the walk, not the decoding,
// is what a launch spends its instructions on (ten gzip -1 files: 32 ms of inflate kernel against 18 for gzip -6 of the same text).
// The chain is a linked list -- lane i's successor is lane i + len_i -- and "which lanes does the list from lane 0 visit" is
// pointer jumping: every lane keeps the set R of lanes its first 2^k steps visit and the lane J it stands on then; six rounds of
// R |= R[J], J = J[J] (three ds_bpermute each) and lane 0 holds the whole chain, however many symbols it has.  A wave-wide prefix
// sum of the symbols' output lengths (DPP) places them in the batch; the first one that does not fit ends the batch.
// ~70 instructions per window whatever it holds, against ~22 per symbol.  MEASURED (profiles/r05_gunzip.txt): no difference --
// ten gzip -1 files 7.98 / 7.90 / 7.87 Gbp/s with the scalar walk / this one behind windows of five symbols or more / this one
// always, BGZF 16.6-17.1 all three: gzip -1 DNA is not literal runs but SHORT MATCHES (2.3 bits per base: ~3 symbols per window,
// where the two walks cost the same), and swapping 66 scalar instructions for 70 vector ones changes nothing because the kernel
// is bound by neither unit's issue rate but by its waves' serial chains.  -- That was with a third of a gzip -1 member's matches
// kept OUT of the walk (their source might lie inside the batch).  Since flush() resolves those (same round) a window's walkable
// symbols doubled, and this walk became the default: inflate_kernel<3> 9.16 -> 7.73 ms per batch of five gzip -1 members, 9.18 ->
// 8.23 at gzip -6 (rocprofv3).  The scalar walk and the mixed mode are gone from the build (round 6); git history has them.
template <int CTRL, int ROW_MASK>
DD_D uint32_t dpp_add(uint32_t x) {
    return x + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
DD_D uint32_t wave_inclusive_sum(uint32_t x) {
    x = dpp_add<0x111, 0xf>(x);   // row_shr:1
    x = dpp_add<0x112, 0xf>(x);   // row_shr:2
    x = dpp_add<0x114, 0xf>(x);   // row_shr:4
    x = dpp_add<0x118, 0xf>(x);   // row_shr:8   -> inclusive sums inside every row of 16
    x = dpp_add<0x142, 0xa>(x);   // row_bcast:15 into rows 1 and 3
    x = dpp_add<0x143, 0xc>(x);   // row_bcast:31 into rows 2 and 3
    return x;
}
// pk: what lane i's symbol is (0: not for the walk; else bits 0..5 its length in bits, 6..14 the bytes it makes).  Out: the
// lanes whose symbols join the batch, each one's slot (osv), the bytes they make, where the walk stands and what it found there
// (pks: 1 = the window is used up, 0 = a symbol the lanes could not finish, else the pk of a symbol the batch has no room for).
DD_D void parallel_walk(uint32_t pk, uint32_t lane, uint32_t used, unsigned long long& mark, uint32_t& pos, uint32_t& outacc, uint32_t& pks, uint32_t& osv) {
    const uint32_t room = 64u - used;
    const bool valid = pk != 0u;
    const uint32_t nxt = lane + (pk & 63u);
    uint32_t J = (valid && nxt < 64u) ? nxt : lane;    // (a lane the walk stops at points at itself)
    uint32_t rlo = lane < 32u ? 1u << lane : 0u, rhi = lane < 32u ? 0u : 1u << (lane - 32u);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t jn = bperm(J, J), a = bperm(J, rlo), b = bperm(J, rhi);
        rlo |= a, rhi |= b;
        J = jn;
    }
    const unsigned long long chain = ((unsigned long long)uni(rhi) << 32) | uni(rlo);   // (lane 0's: the walk starts at the window's first bit)
    const unsigned long long vm = __ballot(valid);
    const uint32_t t = 63u - (uint32_t)__builtin_clzll(chain);   // where the chain ends: a symbol that leaves the window, or one the lanes could not finish
    const bool t_valid = (vm >> t) & 1ull;
    const unsigned long long all = chain & vm;
    const uint32_t ol = ((all >> lane) & 1ull) ? pk >> 6 : 0u;
    const uint32_t incl = wave_inclusive_sum(ol), before = incl - ol;
    const unsigned long long bad = __ballot(ol != 0u && incl > room);
    if (bad) {
        const uint32_t fb = (uint32_t)__builtin_ctzll(bad);
        mark = all & ((1ull << fb) - 1ull);
        pos = fb;
        pks = lane_value(pk, fb);
        outacc = lane_value(before, fb);
    } else {
        mark = all;
        pos = t_valid ? t + (lane_value(pk, t) & 63u) : t;
        pks = t_valid ? 1u : 0u;
        outacc = lane_value(incl, 63u);
    }
    if ((mark >> lane) & 1ull) osv = used + before;
}

// MODE 0: grid = BGZF blocks (jobs), one wave each; the text goes out as bytes, the member's ISIZE and CRC-32 are checked.
// MODE 1 / 2: grid = pieces of single-member gzip files (files / starts): raw deflate data from a block start found by
// find_starts_kernel up to the next one, decoded WITHOUT its 32 KiB of history -- a copy that reaches in front of the
// piece yields placeholders 0x8000 | position in that unknown window (pugz's idea; dd_inflate.h does the same on the
// host).  MODE 3, the one pass nearly every piece needs: 16-bit symbols into the piece's own ranges of the file's symbol
// area (5 x the compressed bytes + 32 Ki symbols per range: DNA inflates 3-4 x), lens[idx] = its text; a piece that
// does not fit (runs of N, repeats) is marked in over[idx] instead and gets MODE 1 -- only count its text -- and, once
// the offsets are known, MODE 2 -- write its symbols into the file's arena at abase[idx].  (Counting EVERY piece first
// and writing dense symbols second cost two full passes: 21 of the 47 ms of ten 50 Mbp files.)
// `errors`: blocks / pieces that could not be decoded (the caller falls back to the host).
template <int MODE>
__global__ __launch_bounds__(64) void inflate_kernel(const InflateJob* __restrict__ jobs, const RawFile* __restrict__ files, int nfiles,
                                                     const uint64_t* __restrict__ starts, uint32_t* __restrict__ lens, uint32_t* __restrict__ over,
                                                     const uint32_t* __restrict__ abase, uint32_t* __restrict__ errors) {
    constexpr bool RAW = MODE != 0;
    constexpr bool WRITES = MODE == 2 || MODE == 3;   // (16-bit symbols)
    bool too_long = false;                             // MODE 3: the piece does not fit its ranges
    constexpr uint32_t kLit = RAW ? 0x40000000u : 0x80000000u;   // a batch lane's source: a literal (else an offset in the text; RAW: negative = in front of the piece)
    const uint32_t lane = threadIdx.x & 63u;
    bool ok = true;
    const uint8_t* in;
    uint32_t n, out_len;
    uint64_t piece_end = ~0ull;
    uint8_t* out = nullptr;
    uint16_t* sym = nullptr;
    PieceRef pr{0, 0, ~0ull, 0, 0};
    if (!RAW) {
        const InflateJob job = jobs[blockIdx.x];
        in = job.in, n = job.in_len, out = job.out, out_len = job.out_len;
    } else {
        if (!piece_of(files, nfiles, starts, blockIdx.x, pr)) {
            if (MODE == 3 && lane == 0) lens[blockIdx.x] = 0, over[blockIdx.x] = 0;
            return;
        }
        if (MODE != 3 && uni(over[blockIdx.x]) == 0u) return;   // (the piece fitted its ranges)
        // (MODE 2 writes into the arena at offsets piece_offsets_kernel made from the counted lengths: a batch that already
        // holds an error -- lengths that do not add up to the member's ISIZE, an arena total beyond it: a damaged or wrapped
        // trailer, `cat a.gz b.gz` -- goes to the host decoder anyway and must not be written)
        if (MODE == 2 && uni(__hip_atomic_load(errors, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0u) return;
        const RawFile rf = files[pr.file];
        in = rf.in, n = rf.in_len, piece_end = pr.end;
        if (MODE == 3) {
            const uint64_t cap = (uint64_t)pr.ranges * rf.range_syms;
            out_len = cap < rf.isize ? (uint32_t)cap : rf.isize;
            sym = rf.sym + (size_t)pr.j * rf.range_syms;
        } else {
            out_len = MODE == 1 ? rf.isize : uni(lens[blockIdx.x]);
            if (MODE == 2) {
                const uint32_t ab = uni(abase[blockIdx.x]);
                if ((uint64_t)ab + out_len > rf.isize) {   // the arena holds ISIZE symbols (piece_offsets_kernel has raised the error already)
                    if (lane == 0) atomicAdd(errors, 1u);
                    return;
                }
                sym = rf.arena + ab;
            }
        }
    }
    uint32_t at = 0;
    // The text goes out 64 bytes at a time: every lane owns one byte of the batch [bstart, bstart + used) and knows where it
    // comes from -- a literal, or an earlier position of the text --, so a batch of ~8 symbols costs ONE load and ONE
    // (contiguous) store, and the serial chain pays a round trip to L2 per batch instead of per symbol.
    uint32_t bstart = 0, used = 0;   // wave-uniform
    uint32_t from = 0;               // this lane's byte: kLit | literal, or its source offset in the text
    auto flush = [&]() {
        if (used) {
            // A lane whose byte comes from INSIDE the batch (a match that starts fewer bytes back than the batch is long: every
            // third match of a gzip -1 member of DNA, round 5) takes over its source lane's source, all lanes at once, until
            // none points into the batch any more: pointer jumping, at most six rounds of one ds_bpermute.  (Round 4 kept such
            // matches out of the lanes' walk and decoded them one at a time.)
            if (MODE != 1) {
                for (;;) {
                    const bool inside = lane < used && !(from & kLit) && (int)from >= (int)bstart;
                    if (!__any(inside)) break;
                    const uint32_t theirs = bperm(inside ? from - bstart : lane, from);
                    if (inside) from = theirs;
                }
            }
            if (MODE == 0) {
                uint32_t v = from & 0xFFu;
                // (what the batch copies was stored by earlier batches of this wave: they have landed before it is read --
                // a batch ago they were issued, the wait is free -- and the bytes are read past the vector L1)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane < used && !(from >> 31)) v = gload1_fresh(out + from);
                if (lane < used) out[bstart + lane] = (uint8_t)v;
            } else if (WRITES) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane < used) {
                    const int f = (int)from;
                    uint32_t v;
                    if (f < 0) v = 0x8000u | (uint32_t)(f + 32768);   // (>= -32768: checked where the copy was met)
                    else if (from & kLit) v = from & 0xFFu;
                    else v = __hip_atomic_load((const DD_GLOBAL uint16_t*)(sym + f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *(DD_GLOBAL uint16_t*)(sym + bstart + lane) = (uint16_t)v;
                }
            }
            bstart += used;
            used = 0;
        }
    };
    // gzip member header: 10 fixed bytes, FEXTRA (BGZF's 'BC' field lives there), then -- not in BGZF, but legal -- name, comment, CRC16
    uint32_t hdr = 0;
    if (!RAW) {
        if (n < 28u || uni(gload1(in)) != 0x1fu || uni(gload1(in + 1)) != 0x8bu || uni(gload1(in + 2)) != 8u) ok = false;
        if (ok) {
            const uint32_t flg = uni(gload1(in + 3));
            hdr = 10;
            if (flg & 4u) hdr += 2u + (uni(gload1(in + 10)) | (uni(gload1(in + 11)) << 8));
            if (flg & (8u | 16u | 2u | 0xE0u)) ok = false;   // (name / comment / header CRC: bgzip writes none; the host decoder takes such files)
            if (hdr + 8u > n) ok = false;
        }
    }
    WBits b;
    bool final_seen = false;
    if (ok) {
        if (!RAW) b.init(in + hdr, n - hdr);
        else {
            b.w = reinterpret_cast<const uint32_t*>(in);   // (the file's bytes start on a 256-byte boundary)
            b.nwords = (n + 3u) / 4u;
            b.start_at((uint32_t)(pr.start >> 5), (uint32_t)pr.start & 31u);
        }
        for (;;) {
            const uint32_t bfinal = b.take(1), btype = b.take(2);
            if (btype == 3u) { ok = false; break; }
            if (btype == 0u) {
                b.drop(b.cnt & 7);
                const uint32_t len = b.take(16), nlen = b.take(16);
                if ((len ^ nlen) != 0xffffu) { ok = false; break; }
                if (at + len > out_len) { ok = false, too_long = true; break; }
                // stored bytes: straight from the input (the reader stands on a byte boundary; its word base stays)
                const uint8_t* const base = reinterpret_cast<const uint8_t*>(b.w);
                const uint32_t data = (uint32_t)(b.bit_pos() >> 3);   // byte offset of the data from the reader's base
                if ((uint32_t)(base - in) + data + len + 8u > n) { ok = false; break; }
                flush();
                if (MODE == 0)
                    for (uint32_t i = lane; i < len; i += 64u) out[at + i] = (uint8_t)gload1(base + data + i);
                if (WRITES)
                    for (uint32_t i = lane; i < len; i += 64u) *(DD_GLOBAL uint16_t*)(sym + at + i) = (uint16_t)gload1(base + data + i);
                bstart = at + len;
                at += len;
                b.start_at((data + len) >> 2, 8u * ((data + len) & 3u));
            } else {
                if (btype == 1u) {
                    for (uint32_t i = lane; i < 320u; i += 64u) g_lds[kLens + i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : i < 288u ? 8 : 5);
                    __builtin_amdgcn_wave_barrier();
                    // (the fixed distance code has 32 codes of 5 bits -- 30 and 31 may not occur, their table entries stay
                    // empty; with 30 the code is incomplete and every fixed block was refused: DD_INFLATE_STRICT found it)
                    if (!uni(build_table(0, 288, 0, kLitInfo, kLitCount, kLitSymbol)) || !uni(build_table(288, 32, 1, kDistInfo, kDistCount, kDistSymbol))) { ok = false; break; }
                } else {
                    if (!dynamic_tables(b)) { ok = false; break; }
                }
                // THE BLOCK'S SYMBOLS, a window of 64 bit positions at a time.
                // A wave issues one instruction in ~4-8 cycles and the waves of a CU share ONE scalar issue slot: a launch
                // of thousands of blocks costs what its scalar instructions cost (the lockstep form -- one table lookup,
                // one set of field extractions, one copy per symbol, all scalar -- ran ~100 scalar instructions per symbol:
                // 5.7 ms per block alone, 13.7 ms for 3 880 blocks; profiles/r04_bgzf.txt).  So the lanes decode: lane i
                // decodes the WHOLE symbol that would start at bit i of the window -- literal/length code, extra bits,
                // distance code, extra bits: two table gathers --; a scalar walk from the symbol that really starts the
                // window follows the chain (one v_readlane and a dozen scalar instructions per symbol) and gives every
                // symbol on it its place in the output batch; then the lanes of the batch look their symbol up and note
                // where their byte comes from.  Symbols the lanes cannot finish alone leave the walk to the one-symbol
                // path below: codes longer than the tables' 10 bits, the end of the block, a match whose source lies before
                // the text's start, one that does not fit a batch.  (Round 4 also sent every match there whose source MIGHT
                // be inside the batch -- distance < length + 64 --: 2 % of the matches of a gzip -6 member of DNA, but 31 % at
                // gzip -1, whose matcher takes the most recent occurrence.  Now flush() resolves sources inside the batch by
                // pointer jumping and they stay in the walk: inflate_kernel<3> over gzip -1 members 12-14 -> ~9 ms per batch,
                // ten 50 Mbp files 8.6 -> 10.9 Gbp/s on one box, 8.6 -> 9.3 on another.)
                uint32_t q, r, s0, s1, s2, s3, s4;   // the window: bit r of word W[q] = s0; s0..s4 = W[q .. q + 4]
                {
                    const uint64_t P = b.bit_pos();
                    q = (uint32_t)(P >> 5);
                    r = (uint32_t)P & 31u;
                    b.seek(q);
                    s0 = b.word(), s1 = b.word(), s2 = b.word(), s3 = b.word(), s4 = b.word();
                }
                uint32_t osv = 0;   // a symbol's lane: the batch slot of its first byte
                for (;;) {
                    // lane i: the 64 bits from bit r + i on
                    const uint32_t x_lo = window32(lane + r, s0, s1, s2, s3), x_hi = window32(lane + r, s1, s2, s3, s4);
                    const uint32_t e1 = l32(kLitInfo + 4u * (x_lo & ((1u << FAST) - 1u)));
                    const uint32_t l1 = e1 & 15u, ex1 = (e1 >> 7) & 15u, kd = (e1 >> 4) & 7u;
                    const uint32_t v1 = (e1 >> 11) + ((x_lo >> l1) & ((1u << ex1) - 1u));   // the literal, or the match's length
                    const uint32_t t1 = l1 + ex1;
                    const uint32_t y = (uint32_t)((((uint64_t)x_hi << 32) | x_lo) >> t1);
                    const uint32_t e2 = l32(kDistInfo + 4u * (y & ((1u << FAST) - 1u)));
                    const uint32_t l2 = e2 & 15u, ex2 = (e2 >> 7) & 15u;
                    const uint32_t dv = (e2 >> 11) + ((y >> l2) & ((1u << ex2) - 1u));
                    // bits 0..5: the symbol's length in bits; 6..14: bytes it makes; 0 = not for the walk
                    uint32_t pk = 0;
                    if (kd == 1u) pk = l1 | (1u << 6);
                    else if (kd == 3u && e2 != 0u && dv <= at + (RAW ? 32768u : 0u)) pk = (t1 + l2 + ex2) | (v1 << 6);
                    unsigned long long mark = 0, starts = 0;
                    uint32_t pos = 0, outacc = 0, pks = 0;
                    parallel_walk(pk, lane, used, mark, pos, outacc, pks, osv);
                    // which slots of the batch start a symbol: the symbols' lanes say so in LDS, the slots' lanes read it back
                    g_lds[kLens + 512u + lane] = 0;
                    __builtin_amdgcn_wave_barrier();
                    if ((mark >> lane) & 1ull) g_lds[kLens + 512u + osv] = 1;
                    __builtin_amdgcn_wave_barrier();
                    starts = __ballot(g_lds[kLens + 512u + lane] != 0);
                    if (outacc) {
                        if (at + outacc > out_len) { ok = false, too_long = true; break; }
                        // the symbols' lanes say where their bytes come from; the batch's lanes find their symbol by counting
                        // (the counting pass of the raw mode needs none of it)
                        if (MODE != 1 && ((mark >> lane) & 1ull)) {
                            const uint32_t rank = lanes_below(mark);
                            const uint32_t src = kd == 1u ? (kLit | v1) : bstart + osv - dv;   // (RAW: may wrap below zero = in front of the piece)
                            *reinterpret_cast<uint2*>(g_lds + kLens + 8u * rank) = make_uint2(src, osv);
                        }
                        __builtin_amdgcn_wave_barrier();
                        if (MODE != 1 && lane - used < outacc) {
                            const uint32_t ord = lanes_below(starts) + (uint32_t)((starts >> lane) & 1ull) - 1u;
                            const uint2 sy = *reinterpret_cast<const uint2*>(g_lds + kLens + 8u * ord);
                            from = sy.x + (lane - sy.y);
                        }
                        __builtin_amdgcn_wave_barrier();
                        used += outacc;
                        at += outacc;
                        if (used == 64u) flush();
                    }
                    if (pos < 64u && pks != 1u) {
                        // ONE SYMBOL, step by step, from the 64 bits at `pos` (a symbol takes at most 15 + 5 + 15 + 13)
                        if (pks != 0u) {   // a match for the walk that does not fit what is left of the batch
                            if (used) {
                                flush();
                                goto advance;
                            }
                        }
                        uint64_t bits = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)x_hi, (int)pos) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)x_lo, (int)pos);
                        const LitLenCode s = litlen_code(bits);
                        if (!s.kind) { ok = false; break; }   // no such code, or one the stream may not use (286, 287)
                        bits >>= s.len, pos += s.len;
                        if (s.kind == 1u) {
                            if (at >= out_len) { ok = false, too_long = true; break; }
                            if (lane == used) from = kLit | s.base;
                            ++at;
                            if (++used == 64u) flush();
                        } else if (s.kind == 2u) {   // end of block
                            flush();
                            r += pos;
                            break;
                        } else {
                            const uint32_t len = s.base + ((uint32_t)bits & ((1u << s.extra) - 1u));
                            bits >>= s.extra, pos += s.extra;
                            // (written out, not a function beside litlen_code: see there)
                            const uint32_t di = uni(l32(kDistInfo + 4u * ((uint32_t)bits & ((1u << FAST) - 1u))));
                            uint32_t dist, dex;
                            if (di) {
                                bits >>= di & 15u, pos += di & 15u;
                                dex = (di >> 7) & 15u;
                                dist = di >> 11;
                            } else {
                                const uint32_t rs = uni(decode_slow(bits, kDistCount, kDistSymbol));
                                const uint32_t ds = rs >> 4;
                                if (rs == ~0u || ds > 29u) { ok = false; break; }
                                bits >>= rs & 15u, pos += rs & 15u;
                                dex = uni((uint32_t)c_dist_extra[ds]);
                                dist = uni((uint32_t)c_dist_base[ds]);
                            }
                            dist += (uint32_t)bits & ((1u << dex) - 1u);
                            pos += dex;
                            if (dist > at + (RAW ? 32768u : 0u)) { ok = false; break; }
                            if (at + len > out_len) { ok = false, too_long = true; break; }
                            // the copy: its bytes join the batch (several batches when it is long).  It reads the dist-byte pattern
                            // in front of it; should that reach into the batch itself, the batch leaves first.
                            const uint32_t pat = at - dist;   // (RAW: may be "negative")
                            at += len;
                            auto place = [&](auto src_of) {
                                uint32_t done = 0;
                                do {
                                    const uint32_t space = 64u - used, left = len - done;
                                    const uint32_t take = left < space ? left : space;
                                    const uint32_t o = done + lane - used;   // this lane's offset inside the match (if it is one of the `take`)
                                    if (MODE != 1 && lane - used < take) from = pat + src_of(o);
                                    used += take;
                                    done += take;
                                    if (used == 64u) flush();
                                } while (done < len);
                            };
                            if (dist >= len) place([](uint32_t o) { return o; });
                            else if (dist == 1u) place([](uint32_t) { return 0u; });   // (a run of N, of one base)
                            else place([&](uint32_t o) { return o % dist; });          // the pattern repeats inside the match
                        }
                    }
                advance:
                    r += pos;
                    while (r >= 32u) {
                        s0 = s1, s1 = s2, s2 = s3, s3 = s4;
                        s4 = b.word();
                        ++q;
                        r -= 32u;
                    }
                }
                if (ok) {   // the reader takes over again where the symbols ended (r may have run past s0)
                    q += r >> 5;
                    b.start_at(q, r & 31u);
                }
                if (!ok) break;
            }
            if (bfinal) {
                final_seen = true;
                break;
            }
            if (RAW) {   // the piece ends where the next one starts -- exactly there, or the starts are not block starts
                const uint64_t P = b.bit_pos();
                if (P == piece_end) break;
                if (P > piece_end) { ok = false; break; }
            }
        }
    }
    if (RAW) {
        if (ok && final_seen != (piece_end == ~0ull)) ok = false;
        if (ok && final_seen && b.bytes_used(in) + 8u != n) ok = false;   // ONE member: CRC-32 and ISIZE right behind the final block
        if (MODE == 3 && !ok && too_long && out_len < files[pr.file].isize) {   // not an error: the piece is counted, then written to the arena
            if (lane == 0) lens[blockIdx.x] = 0, over[blockIdx.x] = 1;
            return;
        }
        if (MODE == 3 && lane == 0) over[blockIdx.x] = 0;
        if ((MODE == 1 || MODE == 3) && lane == 0) lens[blockIdx.x] = ok ? at : 0u;
        if (MODE == 2 && ok && at != out_len) ok = false;
        // (a piece that alone is longer than the member's ISIZE: the trailer's matter -- kSizeMismatch --, not the decoder's)
        if (!ok && lane == 0) {   // (class bits are OR-ed, counts added: 65 536 pieces x 2^16 would add up to zero)
            if (too_long && out_len >= files[pr.file].isize) atomicOr(errors, kSizeMismatch);
            else atomicAdd(errors, 1u);
        }
        return;
    }
    // the member's trailer: CRC-32, ISIZE
    if (ok) {
        const uint32_t used = b.bytes_used(in + hdr);
        if (hdr + used + 8u > n) ok = false;
        else {
            const uint8_t* t = in + hdr + used;
            auto le32 = [&](const uint8_t* q) { return uni(gload1(q)) | (uni(gload1(q + 1)) << 8) | (uni(gload1(q + 2)) << 16) | (uni(gload1(q + 3)) << 24); };
            const uint32_t crc = le32(t), isize = le32(t + 4);
            if (isize != at || at != out_len) ok = false;
            else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the text's last batch has landed
                if (text_crc(out, at) != crc) ok = false;
            }
        }
    }
    if (!ok) {
        if (lane == 0) atomicAdd(errors, 1u);
        return;
    }
}

size_t inflate_lds_bytes() { return kInflateLds; }

void launch_inflate_bgzf(const InflateJob* jobs_dev, int njobs, uint32_t* errors_dev, hipStream_t st) {
    if (njobs <= 0) return;
    hipLaunchKernelGGL(inflate_kernel<0>, dim3((unsigned)njobs), dim3(64), kInflateLds, st, jobs_dev, nullptr, 0, nullptr, nullptr, nullptr, nullptr, errors_dev);
}

void launch_inflate_pieces(int mode, const RawFile* files_dev, int nfiles, int npieces, const uint64_t* starts_dev, uint32_t* lens_dev, uint32_t* over_dev,
                           const uint32_t* abase_dev, uint32_t* errors_dev, hipStream_t st) {
    const auto kernel = mode == 3 ? inflate_kernel<3> : (mode == 1 ? inflate_kernel<1> : inflate_kernel<2>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)npieces), dim3(64), kInflateLds, st, nullptr, files_dev, nfiles, starts_dev, lens_dev, over_dev, abase_dev, errors_dev);
}

}  // namespace dd
