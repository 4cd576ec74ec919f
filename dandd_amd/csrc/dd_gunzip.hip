// dd_gunzip.hip -- ordinary .gz files inflated on the GPU: the pipeline around dd_ginflate.hip's decoder.
//
// ORDINARY .gz files (ONE gzip member: what `gzip` and the sequence archives write) take this file
// (launch_gunzip_members): find_starts_kernel finds deflate block starts by trial, one per 16-128 KiB range of the
// compressed file; the same decoder (inflate_kernel<3>) decodes every piece between two starts WITHOUT the 32 KiB in
// front of it, into 16-bit symbols -- a byte, or "position p of that unknown window"; piece_maps_kernel /
// group_windows_kernel compose the pieces' window-to-window maps in two levels; translate_kernel turns symbols into text
// in the buffer K0 reads; chunk_crc_kernel checks it against the member's CRC-32 (the host combines the chunks).
// Ten 50 Mbp .gz: 12 Gbp/s through dd_sketch_files against 6 with the host decoder; one 3 Gbp .gz: 14.9 against 4.6
// (profiles/r04_gunzip.txt).  Round 5 (profiles/r05_gunzip.txt): several members per file, four-line FASTQ (dd_fastq.hip),
// gzip -1 from 6.7 to 10.7-12.9 Gbp/s, one 400 Mbp member from 8.0 to 11.
// Bit reader, code tables, the one-symbol decoder litlen_code and text_crc are dd_deflate.h's, shared with the decoder.
#include "dd_common.h"
#include "dd_deflate.h"
#include "dd_kernels.h"
#include "dd_scan.h"

namespace dd {

// ---- single-member gzip files: where do deflate blocks start? ---------------------------------------------------
// A wave per guess: file f's guess j covers the bit positions [first_bit + j G, first_bit + (j + 1) G) and reports the
// FIRST position in it that heads a valid dynamic-Huffman block (guess 0 reports first_bit itself).  Lane i tests the
// position base + i: block type 2, HLIT <= 29, HDIST <= 29, the code-length code complete (or a single code) -- 22 % pass
// the first, ~1 % of those the second --; survivors queue up in LDS and are put to the full test 64 at a time, a
// candidate per lane: its code lengths decoded with a bit reader of the lane's own, the literal/length code complete
// with an end-of-block code, the distance code complete or a single code.  What passes that is a block start or a
// one-in-10^9 impostor; an impostor makes a piece end somewhere else than the next one starts and the call goes to the
// host decoder.  Stored and fixed blocks are not looked for (they are decoded as parts of pieces).
constexpr uint32_t kFindTable = kLitInfo;           // u8[64][128]: every lane's code-length code (7-bit lookup): 8 KiB from the symbol tables' place on
constexpr uint32_t kFindQueue = kInflateLds > 8192u ? kInflateLds : 8192u;   // u32[128]: candidate bit positions waiting for the full test (behind the lanes' tables
                                                                              // and behind everything a header parse writes)
constexpr uint32_t kFindLds = kFindQueue + 512u;

__global__ __launch_bounds__(64) void find_starts_kernel(const RawFile* __restrict__ files, int nfiles, uint64_t* __restrict__ starts) {
    const uint32_t lane = threadIdx.x & 63u;
    const RawFile rf = files[file_of(nfiles, blockIdx.x, [&](int f) { return uni(files[f].piece0); })];
    const uint32_t j = blockIdx.x - rf.piece0;
    if (j >= rf.nguess) return;
    if (j == 0) {
        if (lane == 0) starts[blockIdx.x] = rf.first_bit;
        return;
    }
    const uint64_t total_bits = ((uint64_t)rf.in_len - 8u) * 8u;   // (the trailer is no place for a block)
    const uint64_t lo = (uint64_t)rf.first_bit + (uint64_t)j * rf.guess_bits;
    uint64_t found = ~0ull;
    if (lo + 64u < total_bits) {
        const uint64_t hi = lo + rf.guess_bits < total_bits ? lo + rf.guess_bits : total_bits;
        const uint32_t* const W = reinterpret_cast<const uint32_t*>(rf.in);
        const uint32_t nwords = (rf.in_len + 3u) / 4u;
        auto word_at = [&](uint32_t i) { return i < nwords ? gload4(W + i) : 0u; };
        // the full test of up to 64 queued candidates, one per lane; -> the smallest that passes, or ~0u
        auto full_test = [&](uint32_t nq) -> uint64_t {   // (the queue holds positions as offsets from `lo`)
            const uint64_t cand = lo + (lane < nq ? l32(kFindQueue + 4u * lane) : 0u);
            bool live = lane < nq;
            // the lane's bit reader
            uint32_t wi = (uint32_t)(cand >> 5);
            uint64_t buf = ((uint64_t)word_at(wi + 1u) << 32 | word_at(wi)) >> ((uint32_t)cand & 31u);
            int cnt = 64 - (int)((uint32_t)cand & 31u);
            wi += 2u;
            auto need = [&](int k) {
                if (cnt < k) {
                    buf |= (uint64_t)word_at(wi) << cnt;
                    cnt += 32;
                    ++wi;
                }
            };
            auto take = [&](int k) {
                need(k);
                const uint32_t v = (uint32_t)buf & ((1u << k) - 1u);
                buf >>= k, cnt -= k;
                return v;
            };
            (void)take(3);
            const uint32_t hlit = take(5) + 257u, hdist = take(5) + 1u, hclen = take(4) + 4u;
            // its code-length code: lengths, canonical codes, a 128-entry table of its own in LDS
            uint32_t cl[19];
#pragma unroll
            for (int i = 0; i < 19; ++i) cl[i] = 0;
            uint32_t count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 19; ++i) {
                const uint32_t v = (uint32_t)i < hclen ? take(3) : 0u;
#pragma unroll
                for (int s2 = 0; s2 < 19; ++s2)
                    if (c_cl_order[i] == s2) cl[s2] = v;   // (i, s2 unrolled: resolved at compile time)
            }
#pragma unroll
            for (int s2 = 0; s2 < 19; ++s2)
#pragma unroll
                for (int l = 1; l < 8; ++l) count[l] += cl[s2] == (uint32_t)l ? 1u : 0u;
            uint32_t next[8], c = 0;
#pragma unroll
            for (int l = 1; l < 8; ++l) {
                next[l] = c;
                c = (c + count[l]) << 1;
            }
            uint8_t* const tab = g_lds + kFindTable + 128u * lane;
            for (int i = 0; i < 128; i += 4) *reinterpret_cast<uint32_t*>(tab + i) = 0;
#pragma unroll
            for (int s2 = 0; s2 < 19; ++s2) {
                const uint32_t l = cl[s2];
                if (live && l) {
                    uint32_t code = 0;
#pragma unroll
                    for (int q = 1; q < 8; ++q)
                        if (l == (uint32_t)q) code = next[q]++;
                    const uint32_t rev = __builtin_bitreverse32(code) >> (32u - l);
                    for (uint32_t e = rev; e < 128u; e += 1u << l) tab[e] = (uint8_t)(l | ((uint32_t)s2 << 3));
                }
            }
            // the literal/length and distance code lengths, run-length coded: Kraft sums in units of 2^-15
            const uint32_t totalsym = hlit + hdist;
            uint32_t i = 0, prev = 0, kraft_ll = 0, kraft_d = 0, nz_d = 0, eob = 0;
            while (__any(live && i < totalsym)) {
                if (live && i < totalsym) {
                    need(14);
                    const uint32_t e = tab[(uint32_t)buf & 127u];
                    if (!e) live = false;
                    else {
                        buf >>= e & 7u, cnt -= (int)(e & 7u);
                        const uint32_t sy = e >> 3;
                        uint32_t rep = 1, val = sy;
                        if (sy == 16u) {
                            if (!i) live = false;
                            val = prev;
                            rep = 3u + ((uint32_t)buf & 3u);
                            buf >>= 2, cnt -= 2;
                        } else if (sy == 17u) {
                            val = 0;
                            rep = 3u + ((uint32_t)buf & 7u);
                            buf >>= 3, cnt -= 3;
                        } else if (sy == 18u) {
                            val = 0;
                            rep = 11u + ((uint32_t)buf & 127u);
                            buf >>= 7, cnt -= 7;
                        }
                        if (i + rep > totalsym) live = false;
                        if (live && val) {
                            const uint32_t n_ll = i < hlit ? (hlit - i < rep ? hlit - i : rep) : 0u, n_d = rep - n_ll;
                            kraft_ll += n_ll << (15u - val);
                            kraft_d += n_d << (15u - val);
                            nz_d += n_d;
                            if (i <= 256u && 256u < i + rep) eob = val;
                        }
                        i += rep;
                        prev = val;
                    }
                }
            }
            const bool pass = live && eob != 0u && kraft_ll == (1u << 15) && (kraft_d == (1u << 15) || nz_d <= 1u) && hlit <= 286u && hdist <= 30u;
            // What passes is a block start or, once in ~10^9 positions, an impostor (8 x 50 Mbp of gzip -6 held one).  The
            // last word has a trial decoding, wave-uniform, with the decoder's own tables: the header parsed again, then
            // the first symbols -- every code valid, every literal a byte of text (9 .. 126: FASTA has no others).
            unsigned long long m = __ballot(pass);
            while (m) {
                const int first = __builtin_ctzll(m);
                const uint64_t c0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cand >> 32), first) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cand, first);
                m &= m - 1ull;
                WBits v;
                v.w = W, v.nwords = nwords;
                v.start_at((uint32_t)(c0 >> 5), (uint32_t)c0 & 31u);
                (void)v.take(3);
                bool good = dynamic_tables(v);
                for (int k = 0; good && k < 24; ++k) {
                    v.need();
                    const LitLenCode s = litlen_code(v.buf);
                    if (!s.kind) { good = false; break; }
                    v.drop((int)s.len);
                    if (s.kind == 1u && (s.base < 9u || s.base > 126u)) good = false;
                    if (s.kind == 2u) break;
                    if (s.kind == 3u) {
                        v.drop((int)s.extra);
                        v.need();
                        const uint32_t di = uni(l32(kDistInfo + 4u * v.peek(FAST)));
                        if (di) v.drop((int)((di & 15u) + ((di >> 7) & 15u)));
                        else {
                            const uint32_t r = uni(decode_slow(v.buf, kDistCount, kDistSymbol));
                            if (r == ~0u || (r >> 4) > 29u) { good = false; break; }
                            v.drop((int)(r & 15u));
                            v.need();
                            v.drop((int)uni((uint32_t)c_dist_extra[r >> 4]));
                        }
                    }
                }
                if (good) return c0;
            }
            return ~0ull;
        };
        // Kraft sum and count of the code-length code's non-zero lengths, three 3-bit lengths at a time: a 512-entry table at the
        // front of LDS (round 5; the unrolled 19-length sum was ~95 of the scan's ~110 VALU instructions per 64 positions, and the
        // scan is what this kernel's 5 ms per batch were made of).  full_test() overwrites it with its own tables: rebuilt after.
        auto build_lut = [&]() {
            for (uint32_t v = lane; v < 512u; v += 64u) {
                uint32_t kr = 0, nzv = 0;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t l = (v >> (3 * q)) & 7u;
                    kr += l ? (128u >> l) : 0u;
                    nzv += l ? 1u : 0u;
                }
                l32(kLitInfo + 4u * v) = kr | (nzv << 16);
            }
            __builtin_amdgcn_wave_barrier();
        };
        build_lut();
        uint32_t nq = 0;
        // The stream comes in through ONE load per 29 steps: lane l holds word cbase + l of a 64-word chunk, a step takes the six
        // words its 64 positions span out of it with v_readlane (the step's first word is wave-uniform) and every lane picks its
        // three by the word its position starts in.  (Four loads per lane and step, each behind a bounds check and a 64-bit
        // address, were what the scan waited for: round 5, profiles/r05_gunzip.txt.)
        uint32_t cbase = (uint32_t)(lo >> 5), cw = word_at(cbase + lane);
        const uint32_t r0 = (uint32_t)lo & 31u;   // (base = lo + 64 n: its bit inside its word never changes)
        const uint32_t tt = lane + r0;
        for (uint64_t base = lo; base < hi && found == ~0ull; base += 64u) {
            // the 96 bits from position base + lane on
            const uint64_t pos = base + lane;
            uint32_t qrel = (uint32_t)(base >> 5) - cbase;
            if (qrel + 5u > 63u) {
                cbase += qrel;
                cw = word_at(cbase + lane);
                qrel = 0;
            }
            const uint32_t s0 = lane_value(cw, qrel), s1 = lane_value(cw, qrel + 1u), s2 = lane_value(cw, qrel + 2u), s3 = lane_value(cw, qrel + 3u),
                           s4 = lane_value(cw, qrel + 4u), s5 = lane_value(cw, qrel + 5u);
            const uint32_t x0 = window32(tt, s0, s1, s2, s3), x1 = window32(tt, s1, s2, s3, s4), x2 = window32(tt, s2, s3, s4, s5);
            const uint32_t hclen = ((x0 >> 13) & 15u) + 4u;
            bool cand = pos < hi && ((x0 >> 1) & 3u) == 2u && ((x0 >> 3) & 31u) <= 29u && ((x0 >> 8) & 31u) <= 29u;
            // Kraft sum of the code-length code (3-bit lengths from bit 17 on, the first hclen of them) in units of 2^-7
            const uint32_t f_lo = __builtin_amdgcn_alignbit(x1, x0, 17), f_hi = __builtin_amdgcn_alignbit(x2, x1, 17);
            const uint32_t nbits = 3u * hclen;   // 12 .. 57
            const uint32_t fa = f_lo & (nbits >= 32u ? ~0u : (1u << (nbits & 31u)) - 1u), fb = f_hi & (nbits > 32u ? (1u << ((nbits - 32u) & 31u)) - 1u : 0u);
            auto lut = [&](uint32_t nine) { return l32(kLitInfo + 4u * (nine & 511u)); };
            const uint32_t sum = lut(fa) + lut(fa >> 9) + lut(fa >> 18) + lut((fa >> 27) | (fb << 5)) + lut(fb >> 4) + lut(fb >> 13) + lut(fb >> 22);
            const uint32_t kraft = sum & 0xFFFFu, nz = sum >> 16;
            cand = cand && (kraft == 128u || nz == 1u);
            const unsigned long long m = __ballot(cand);
            if (m) {
                if (cand) l32(kFindQueue + 4u * (nq + lanes_below(m))) = (uint32_t)(pos - lo);
                nq += (uint32_t)__builtin_popcountll(m);
                __builtin_amdgcn_wave_barrier();
                if (nq >= 64u) {
                    found = full_test(64u);
                    __builtin_amdgcn_wave_barrier();
                    build_lut();
                    // the rest of the queue moves to the front
                    const uint32_t restv = lane < nq - 64u ? l32(kFindQueue + 4u * (64u + lane)) : 0u;
                    __builtin_amdgcn_wave_barrier();
                    if (lane < nq - 64u) l32(kFindQueue + 4u * lane) = restv;
                    nq -= 64u;
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (found == ~0ull && nq) found = full_test(nq);
    }
    if (lane == 0) starts[blockIdx.x] = found;
}

// text offsets of the pieces (one wave per file; <= a few thousand pieces): offs[i] = sum of the lens before i; the sum
// must be the member's ISIZE
// ... and abase[i] = the same sum over the pieces that go to the arena
__global__ __launch_bounds__(64) void piece_offsets_kernel(const RawFile* __restrict__ files, const uint32_t* __restrict__ lens, const uint32_t* __restrict__ over,
                                                           uint32_t* __restrict__ offs, uint32_t* __restrict__ abase, uint32_t* __restrict__ errors) {
    const RawFile rf = files[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    // (64-bit sums: a piece's length is bounded by ISIZE, their SUM is not -- a trailer whose ISIZE is smaller than the text
    // (damage, two members, a text beyond 4 GiB whose ISIZE is the length mod 2^32) must not wrap back into "equal")
    uint64_t run = 0, arun = 0;
    for (uint32_t b0 = 0; b0 < rf.nguess; b0 += 64u) {
        const uint32_t i = b0 + lane, mine = i < rf.nguess ? lens[rf.piece0 + i] : 0u, amine = (i < rf.nguess && over[rf.piece0 + i]) ? mine : 0u;
        const uint64_t incl = wave_incl_sum<uint64_t>(mine), aincl = wave_incl_sum<uint64_t>(amine);
        // (offsets beyond ISIZE are clamped: nothing reads them once the error below is up, and nothing may index with a wrapped one)
        const uint64_t o = run + incl - mine, a = arun + aincl - amine;
        if (i < rf.nguess) offs[rf.piece0 + i] = (uint32_t)(o < rf.isize ? o : rf.isize), abase[rf.piece0 + i] = (uint32_t)(a < rf.isize ? a : rf.isize);
        run += (uint64_t)__shfl((long long)incl, 63);
        arun += (uint64_t)__shfl((long long)aincl, 63);
    }
    // kSizeMismatch: the pieces decoded, but not to the text the trailer announces (the host tells this from a refused block)
    if ((run != (uint64_t)rf.isize || arun > (uint64_t)rf.isize) && lane == 0) atomicOr(errors, kSizeMismatch);
}

// where a piece's symbols are: its ranges of the symbol area, or the arena
DD_D const uint16_t* piece_symbols(const RawFile& rf, uint32_t i, const uint32_t* over, const uint32_t* abase) {
    return over[rf.piece0 + i] ? rf.arena + abase[rf.piece0 + i] : rf.sym + (size_t)i * rf.range_syms;
}

// What stands in the 32 KiB in front of every piece?  Piece i turns the window in front of it into the window behind it:
// every position of the new window is a byte of the piece or a position of the old window -- a MAP of 32 768 16-bit
// entries, and maps compose.  Walking a file's pieces one after the other with the window in LDS cost ~7 us a piece on ONE
// CU (52 of the 241 ms of a 3 Gbp assembly's 7 500 pieces) while the chip waited.  Two levels instead:
//   piece_maps_kernel     a workgroup per GROUP of 32 ranges, all groups of all files side by side: starting from the
//                         identity, compose the group's pieces; the map in front of each piece (relative to the group's
//                         start) is stored, and the group's whole map at the end
//   group_windows_kernel  a workgroup per file walks its GROUPS (a 32nd of the steps): the window at each group's start
//   translate_kernel      a placeholder goes through its piece's map and, if that still points in front of the group, through
//                         the group's window
// A thread owns the window positions t, t + 1024, ..: a wave's symbol loads are 128 contiguous bytes, and a step's symbols
// are asked for a step ahead (the chain waits for LDS and a barrier per piece, not for HBM).
DD_D uint16_t* piece_map(const RawFile& rf, uint32_t i) { return reinterpret_cast<uint16_t*>(rf.windows) + (size_t)i * 32768u; }
DD_D uint16_t* group_map(const RawFile& rf, uint32_t g) { return reinterpret_cast<uint16_t*>(rf.windows) + ((size_t)rf.nguess + g) * 32768u; }
DD_D uint8_t* group_window(const RawFile& rf, uint32_t g) { return rf.windows + ((size_t)rf.nguess + rf.ngroups) * 65536u + (size_t)g * 32768u; }

__global__ __launch_bounds__(1024) void piece_maps_kernel(const RawFile* __restrict__ files, int nfiles, const uint32_t* __restrict__ lens,
                                                          const uint32_t* __restrict__ over, const uint32_t* __restrict__ abase, const uint32_t* __restrict__ errors) {
    extern __shared__ __attribute__((aligned(16))) uint8_t win[];   // u16 [2][32768]
    if (*errors) return;   // (a refused batch: lengths and offsets may not fit each other; the call goes to the host anyway)
    const RawFile rf = files[file_of(nfiles, blockIdx.x, [&](int f) { return files[f].group0; })];
    const uint32_t g = blockIdx.x - rf.group0;
    if (g >= rf.ngroups) return;
    const uint32_t first = g * kPieceGroup, last = first + kPieceGroup < rf.nguess ? first + kPieceGroup : rf.nguess;
    uint16_t* maps = reinterpret_cast<uint16_t*>(win);
    const uint32_t t0 = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 32; ++q) maps[t0 + 1024u * q] = (uint16_t)(0x8000u | (t0 + 1024u * q));   // the identity
    __syncthreads();
    auto next_piece = [&](uint32_t i) {   // first piece with text at or behind i
        while (i < last && lens[rf.piece0 + i] == 0u) ++i;
        return i;
    };
    uint16_t cur_s[32], nxt_s[32];
    auto fetch = [&](uint32_t i, uint16_t (&dst)[32]) {
        if (i >= last) return;
        const uint32_t L = lens[rf.piece0 + i];
        const uint16_t* const s = piece_symbols(rf, i, over, abase);
        const int p0 = (int)L - 32768 + (int)t0;
#pragma unroll
        for (int q = 0; q < 32; ++q) dst[q] = (p0 + 1024 * q >= 0) ? s[p0 + 1024 * q] : (uint16_t)0;
    };
    uint32_t i = next_piece(first), cur = 0;
    fetch(i, cur_s);
    while (i < last) {
        const uint32_t L = lens[rf.piece0 + i], inext = next_piece(i + 1u);
        fetch(inext, nxt_s);
        uint16_t* const before = piece_map(rf, i);
        const uint16_t* const w = maps + cur * 32768u;
        uint16_t* const nw = maps + (cur ^ 1u) * 32768u;
#pragma unroll
        for (int q = 0; q < 16; ++q) reinterpret_cast<uint32_t*>(before)[t0 + 1024u * q] = reinterpret_cast<const uint32_t*>(w)[t0 + 1024u * q];
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const uint32_t pos = t0 + 1024u * q;
            const int p = (int)L - 32768 + (int)pos;
            const uint32_t sy = cur_s[q];
            nw[pos] = (uint16_t)(p >= 0 ? ((sy & 0x8000u) ? (uint32_t)w[sy & 0x7fffu] : sy) : (uint32_t)w[pos + L]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 32; ++q) cur_s[q] = nxt_s[q];
        cur ^= 1u;
        i = inext;
    }
    uint16_t* const gm = group_map(rf, g);
    const uint16_t* const w = maps + cur * 32768u;
#pragma unroll
    for (int q = 0; q < 16; ++q) reinterpret_cast<uint32_t*>(gm)[t0 + 1024u * q] = reinterpret_cast<const uint32_t*>(w)[t0 + 1024u * q];
}

__global__ __launch_bounds__(1024) void group_windows_kernel(const RawFile* __restrict__ files, const uint32_t* __restrict__ errors) {
    extern __shared__ __attribute__((aligned(16))) uint8_t win[];   // u8 [2][32768]
    if (*errors) return;
    const RawFile rf = files[blockIdx.x];
    const uint32_t t0 = threadIdx.x;
    for (uint32_t t = t0; t < 32768u / 4u; t += 1024u) reinterpret_cast<uint32_t*>(win)[t] = 0;   // nothing stands in front of the stream
    __syncthreads();
    uint16_t cur_m[32], nxt_m[32];
    auto fetch = [&](uint32_t g, uint16_t (&dst)[32]) {
        if (g >= rf.ngroups) return;
        const uint16_t* const m = group_map(rf, g);
#pragma unroll
        for (int q = 0; q < 32; ++q) dst[q] = m[t0 + 1024u * q];
    };
    uint32_t cur = 0;
    fetch(0, cur_m);
    for (uint32_t g = 0; g < rf.ngroups; ++g) {
        fetch(g + 1u, nxt_m);
        uint8_t* const at_start = group_window(rf, g);
        const uint8_t* const w = win + cur * 32768u;
        uint8_t* const nw = win + (cur ^ 1u) * 32768u;
#pragma unroll
        for (int q = 0; q < 8; ++q) reinterpret_cast<uint32_t*>(at_start)[t0 + 1024u * q] = reinterpret_cast<const uint32_t*>(w)[t0 + 1024u * q];
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const uint32_t v = cur_m[q];
            nw[t0 + 1024u * q] = (uint8_t)((v & 0x8000u) ? (uint32_t)w[v & 0x7fffu] : v);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 32; ++q) cur_m[q] = nxt_m[q];
        cur ^= 1u;
    }
}

// symbols -> text: one workgroup per 64 KiB of a file's text; a placeholder is looked up in the map in front of its piece and, if
// that points in front of the piece's group, in the window at the group's start
__global__ __launch_bounds__(256) void translate_kernel(const RawFile* __restrict__ files, int nfiles, const uint32_t* __restrict__ chunk0,
                                                        const uint32_t* __restrict__ lens, const uint32_t* __restrict__ offs, const uint32_t* __restrict__ over,
                                                        const uint32_t* __restrict__ abase, const uint32_t* __restrict__ errors) {
    if (*errors) return;
    const int f = file_of(nfiles, blockIdx.x, [&](int i) { return chunk0[i]; });
    const RawFile rf = files[f];
    const uint32_t c = blockIdx.x - chunk0[f], begin = c * 65536u, end = begin + 65536u < rf.isize ? begin + 65536u : rf.isize;
    if (begin >= rf.isize) return;
    // the piece that holds `begin`: the last one with offs <= begin and a text of its own (binary search, then a few steps)
    uint32_t lo = 0, hi = rf.nguess;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (offs[rf.piece0 + mid] <= begin) lo = mid;
        else hi = mid;
    }
    // (round 5: the piece's offset, end and symbols stay in registers until a position leaves the piece -- the first form
    // re-read lens / offs / over / abase in front of every symbol, three dependent loads on a chain of five -- and four positions
    // go per step, their loads side by side: 2.42 -> 1.13 ms for 400 MB of text; the kernel waits for memory latency, not bandwidth)
    uint32_t pi = lo, off = offs[rf.piece0 + pi], pend = off + lens[rf.piece0 + pi];
    const uint16_t* syms = piece_symbols(rf, pi, over, abase);
    auto settle = [&](uint32_t p) {   // the piece that holds position p (pieces without a text of their own are stepped over)
        while (pi + 1u < rf.nguess && p >= pend) {
            ++pi;
            off = offs[rf.piece0 + pi];
            pend = off + lens[rf.piece0 + pi];
            syms = piece_symbols(rf, pi, over, abase);
        }
    };
    auto resolve = [&](uint32_t sy, uint32_t piece) {
        if (sy & 0x8000u) {
            sy = piece_map(rf, piece)[sy & 0x7fffu];
            if (sy & 0x8000u) sy = group_window(rf, piece / kPieceGroup)[sy & 0x7fffu];
        }
        return sy;
    };
    uint32_t p = begin + threadIdx.x;
    for (; p + 768u < end; p += 1024u) {
        settle(p);
        if (p + 768u < pend) {   // all four in this piece: four independent loads
            uint32_t sy[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sy[q] = syms[p + 256u * q - off];
#pragma unroll
            for (int q = 0; q < 4; ++q) rf.text[p + 256u * q] = (uint8_t)resolve(sy[q], pi);
        } else {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                settle(p + 256u * q);
                rf.text[p + 256u * q] = (uint8_t)resolve(syms[p + 256u * q - off], pi);
            }
        }
    }
    for (; p < end; p += 256u) {
        settle(p);
        rf.text[p] = (uint8_t)resolve(syms[p - off], pi);
    }
}

// CRC-32 of every 64 KiB of the texts (one wave each): the host combines them (zlib's crc32_combine) and compares with the trailer's
__global__ __launch_bounds__(64) void chunk_crc_kernel(const RawFile* __restrict__ files, int nfiles, const uint32_t* __restrict__ chunk0, uint32_t* __restrict__ crcs,
                                                       const uint32_t* __restrict__ errors) {
    if (*errors) return;
    const int f = file_of(nfiles, blockIdx.x, [&](int i) { return uni(chunk0[i]); });
    const RawFile rf = files[f];
    const uint32_t c = blockIdx.x - uni(chunk0[f]), begin = c * 65536u;
    if (begin >= rf.isize) return;
    const uint32_t n = rf.isize - begin < 65536u ? rf.isize - begin : 65536u;
    const uint32_t crc = text_crc(rf.text + begin, n);
    if ((threadIdx.x & 63u) == 0u) crcs[blockIdx.x] = crc;
}

// Single-member gzip files on the device: block starts -> piece lengths -> offsets -> symbols -> windows -> text -> CRCs.
// npieces = sum of the files' nguess; nchunks = sum of their 64 KiB text chunks (chunk0_dev: first chunk of each file, nfiles + 1 entries).
void launch_gunzip_members(const RawFile* files_dev, int nfiles, int npieces, int ngroups, int nchunks, uint64_t* starts, uint32_t* tables_dev, size_t stride,
                           const uint32_t* chunk0_dev, uint32_t* crcs_dev, uint32_t* errors_dev, hipStream_t st) {
    if (nfiles <= 0 || npieces <= 0) return;
    uint32_t *lens = tables_dev, *offs = tables_dev + stride, *over = tables_dev + 2 * stride, *abase = tables_dev + 3 * stride;
    const dim3 grid((unsigned)npieces), wave(64);
    hipLaunchKernelGGL(find_starts_kernel, grid, wave, kFindLds, st, files_dev, nfiles, starts);
    launch_inflate_pieces(3, files_dev, nfiles, npieces, starts, lens, over, nullptr, errors_dev, st);
    launch_inflate_pieces(1, files_dev, nfiles, npieces, starts, lens, over, nullptr, errors_dev, st);   // (the pieces marked in `over` only)
    hipLaunchKernelGGL(piece_offsets_kernel, dim3((unsigned)nfiles), wave, 0, st, files_dev, lens, over, offs, abase, errors_dev);
    launch_inflate_pieces(2, files_dev, nfiles, npieces, starts, lens, over, abase, errors_dev, st);
    launch_full_lds<piece_maps_kernel>(dim3((unsigned)ngroups), dim3(1024), 131072, st, files_dev, nfiles, lens, over, abase, errors_dev);
    launch_full_lds<group_windows_kernel>(dim3((unsigned)nfiles), dim3(1024), 65536, st, files_dev, errors_dev);
    if (nchunks > 0) {
        hipLaunchKernelGGL(translate_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, files_dev, nfiles, chunk0_dev, lens, offs, over, abase, errors_dev);
        hipLaunchKernelGGL(chunk_crc_kernel, dim3((unsigned)nchunks), wave, kInflateLds, st, files_dev, nfiles, chunk0_dev, crcs_dev, errors_dev);
    }
}

}  // namespace dd
