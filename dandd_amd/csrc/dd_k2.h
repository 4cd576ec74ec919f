// dd_k2.h -- what the register-slab (K2) kernels share: the privatised LDS histogram image, the SWAR byte helpers, the bit
// slicer of the plane kernels, and the correction form (hist = base + corr) of dd_leaveout.hip and dd_extend.hip with its
// launch shape.  Device code, plus the few host helpers that launch it.
#pragma once
#include "dd_common.h"

namespace dd {

// ---- bytes: four HLL registers (<= 63) per dword, sixteen per 16-byte piece -------------------------------------------
DD_D uint4 bmax16(uint4 a, uint4 b) {
    return make_uint4(bmax4(a.x, b.x), bmax4(a.y, b.y), bmax4(a.z, b.z), bmax4(a.w, b.w));
}

DD_D uint32_t bmin4(uint32_t a, uint32_t b) {
    const uint32_t t = (a | 0x80808080u) - b;
    const uint32_t m = ((t >> 7) & 0x01010101u) * 0xFFu;  // 0xFF where a >= b
    return (b & m) | (a & ~m);
}

// bit 7 of each byte: a > b (128 + a - b - 1 stays within 64..190: no borrow between bytes)
DD_D uint32_t bgt4(uint32_t a, uint32_t b) { return ((a | 0x80808080u) - b - 0x01010101u) & 0x80808080u; }

// the four words of a piece, every byte cut to a register's six bits
DD_D void unpack16(const uint4& v, uint32_t (&w)[4]) {
    w[0] = v.x & 0x3f3f3f3fu, w[1] = v.y & 0x3f3f3f3fu, w[2] = v.z & 0x3f3f3f3fu, w[3] = v.w & 0x3f3f3f3fu;
}

// the six bit planes of 32 registers (8 dwords of 4 bytes): bit i + 8 q of plane b = bit b of byte q of dword i
DD_D void bit_slice(const uint32_t (&w)[8], uint32_t (&pl)[6]) {
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t s = i >= b ? w[i] << (i - b) : w[i] >> (b - i);
            acc |= s & (0x01010101u << i);
        }
        pl[b] = acc;
    }
}

// ---- the histogram image -----------------------------------------------------------------------------------------------
// kHistWords u32 of LDS, a static __shared__ array or the head of a dynamic block: h[bin][copy], copy = lane % 32.
// ds_add_u32 is serviced in two groups of 32 lanes, each over 32 banks of 4 bytes: with the copy as the fastest index every
// lane of a group adds into ITS OWN bank whatever bins the bytes name -- no bank conflict is possible (lanes l and l + 32
// share a copy but not a group).  The copy-major image this replaces (h[copy][65]) put (copy + bin) % 32 on the bank: ~3.5
// lanes of a group collided on average.
constexpr int kHistCopies = 32;  // privatised LDS histograms per workgroup
constexpr int kHistWords = 64 * kHistCopies;

// (indexed as the two-dimensional array it is: for bin * kHistCopies + copy the compiler forms its addresses another way)
DD_D uint32_t& hist_at(uint32_t* h, uint32_t bin, uint32_t copy) { return reinterpret_cast<uint32_t(*)[kHistCopies]>(h)[bin][copy]; }

DD_D void hist_zero(uint32_t* h) {
    for (int i = threadIdx.x; i < kHistWords; i += blockDim.x) h[i] = 0;
}

DD_D void hist_add(uint32_t* h, uint32_t bin) { atomicAdd(&hist_at(h, bin, threadIdx.x & (kHistCopies - 1)), 1u); }

// add the 16 register bytes of w to the workgroup's privatised histograms
DD_D void hist_add16(uint32_t* h, const uint32_t (&w)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 4; ++b) hist_add(h, (w[q] >> (8 * b)) & 63u);
    }
}
DD_D void hist_add16(uint32_t* h, uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    hist_add16(h, w);
}

// fold the privatised copies and add them to a global 64-bin histogram (exclusive: the row has no other writer)
DD_D void hist_flush(uint32_t* h, uint32_t* __restrict__ gh, bool exclusive) {
    if (threadIdx.x < 64) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kHistCopies; ++c) s += hist_at(h, threadIdx.x, (c + threadIdx.x) & (kHistCopies - 1));  // (rotated: thread t starts at bank t)
        if (exclusive)
            gh[threadIdx.x] = s;
        else if (s)
            atomicAdd(&gh[threadIdx.x], s);
    }
}

// ---- the correction form -----------------------------------------------------------------------------------------------
// hist[(r * K + kk) * 64 + bin] = base + corr_r for the rows r < nrows of a schedule, u32 counts mod 2^32: a bin of corr_r never
// goes below -base[bin].  A workgroup's dynamic LDS is the image of base (counted by the first row tile only), then
// corr[row][64][copies]; it flushes once, one global atomic per non-zero bin, base into row nrows; launch_corr_finish then
// adds row nrows to the rows before it.
constexpr int kCorrThreads = 512;
constexpr int kCorrTile = 256;   // rows (times copies) whose corrections one workgroup keeps in LDS: 64 KiB + 8 KiB, two workgroups per CU

inline size_t corr_lds_bytes(int slots) { return sizeof(uint32_t) * (kHistWords + (size_t)slots * 64); }

DD_D uint32_t* corr_of(uint32_t* lds) { return lds + kHistWords; }

DD_D void corr_zero(uint32_t* lds, int slots) {
    for (int i = threadIdx.x; i < kHistWords + slots * 64; i += blockDim.x) lds[i] = 0;
}

// after the barrier that ends the counting: rows r0 .. r0 + count - 1 of column kk get their corrections (the sum of
// their `copies`; leave-out keeps one), row nrows the image where this workgroup counted it
DD_D void corr_flush(uint32_t* lds, bool count_full, int r0, int count, int copies, int nrows, int K, int kk,
                     uint32_t* __restrict__ hist) {
    if (count_full) hist_flush(lds, hist + ((size_t)nrows * K + kk) * 64, false);
    const uint32_t* corr = corr_of(lds);
    for (int i = threadIdx.x; i < count * 64; i += blockDim.x) {
        uint32_t v = 0;
        for (int c = 0; c < copies; ++c) v += corr[(size_t)i * copies + c];
        if (v) atomicAdd(&hist[((size_t)(r0 + i / 64) * K + kk) * 64 + (i & 63)], v);
    }
}

// host: a correction kernel's grid is (row tile, k, tile), a workgroup taking every tiles-th 16-byte piece of its k column
struct CorrShape {
    int threads, tiles;
};
inline CorrShape corr_shape(int p, int K, int row_tiles) {
    const size_t m16 = ((size_t)1 << p) >> 4;
    const int threads = (int)(m16 < (size_t)kCorrThreads ? (m16 < 64 ? 64 : m16) : kCorrThreads);
    // about four workgroups per CU over the whole grid (two resident at a time), never more than one piece per thread
    const size_t most = (m16 + threads - 1) / threads;
    size_t tiles = (1024 + (size_t)K * row_tiles - 1) / ((size_t)K * row_tiles);
    if (tiles > most) tiles = most;
    if (tiles < 1) tiles = 1;
    return {threads, (int)tiles};
}

}  // namespace dd
