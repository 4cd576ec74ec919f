// dd_extend.hip -- K2 extend unions: the register histogram of "base U leaf_g" for every candidate leaf g from ONE read of
// the candidates' rows.
//
// The question behind `dandd greedy` (steepest / flattest growth orderings): given the union of the genomes chosen so far
// (`base`, a sketch that is no leaf), what would each remaining genome make of it?  Per (candidate, k) that is the 64-bin
// histogram of the byte-max of base and the candidate's row.
//
// Corrections, as dd_leaveout.hip:
//         hist(base U leaf_g) = hist(base) + corr_g,
//         corr_g[leaf_g[r]] += 1, corr_g[base[r]] -= 1   for every register r with leaf_g[r] > base[r],
// exact integers (u32 arithmetic mod 2^32: a bin of corr_g never goes below -hist(base)[bin]).  A thread keeps a 16-byte
// piece of base in VGPRs and the candidates' pieces stream past it, kUnroll rows in flight; "greater than" is the SWAR
// borrow trick of leaveout_kernel (bytes <= 63).  hist(base) itself is counted by candidate tile 0 in an LDS image
// privatised 32 ways (dd_union.hip's: h[bin][copy]).
//
// The corrections of up to kTileC = 256 candidates sit in LDS as corr[candidate][64][copies] u32 (64 KiB + 8 KiB: two
// workgroups per CU); with fewer candidates some of the room goes to `copies` (a power of two, copy = lane % copies),
// which cuts the lanes that meet on one word when base is small and most registers correct -- the first steps of a walk
// over unrelated genomes, the only ones that are LDS-atomic-bound (profiles/greedy_extend.txt).  More candidates are cut into tiles of 256, one grid slice each.  A workgroup flushes once, one
// global atomic per non-zero bin; extend_finish_kernel adds hist(base) to every candidate row.
//
// An EMPTY base needs no corrections at all (every non-zero register would be one): rows_hist_kernel counts the listed
// rows' own histograms, dd_union.hip's hist_kernel over a row list.
#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kTileC = 256;      // candidates (times copies) whose corrections one workgroup keeps in LDS
constexpr int kCopySlots = 160;  // ... and what `copies` may widen them to
constexpr int kECopies = 32;     // privatised copies of base's own histogram
constexpr int kEThreads = 512;
constexpr int kEUnroll = 8;      // candidate rows in flight per thread

// grid: blockIdx.x = (ctile * K + kk) * tiles + tile; a workgroup takes every tiles-th 16-byte piece of k column kk
// hist[(r * K + kk) * 64 + bin]: corrections of candidate slot r < nrows; row nrows: base's own histogram
__global__ __launch_bounds__(kEThreads) void extend_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ leaf,
                                                           int K, int p, const int32_t* __restrict__ rows, int nrows, int tiles,
                                                           int copies, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lds[];            // full[64][kECopies], then corr[ccount][64][copies]
    uint32_t* full = lds;
    uint32_t* corr = lds + 64 * kECopies;
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int ctile = blockIdx.x / tiles / K;
    const int per_tile = kTileC / copies;
    const int c0 = ctile * per_tile;
    const int ccount = nrows - c0 < per_tile ? nrows - c0 : per_tile;
    const bool count_full = ctile == 0;
    for (int i = threadIdx.x; i < 64 * kECopies + ccount * 64 * copies; i += blockDim.x) lds[i] = 0;
    __syncthreads();

    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t row_stride = (size_t)K << p;    // bytes from one leaf's row kk to the next leaf's
    const uint8_t* col = leaf + ((size_t)kk << p);
    const uint8_t* bcol = base + ((size_t)kk << p);
    const int copy = threadIdx.x & (kECopies - 1);
    const int cp = threadIdx.x & (copies - 1);
    for (size_t piece = (size_t)tile * blockDim.x + threadIdx.x; piece < m16; piece += (size_t)tiles * blockDim.x) {
        const uint8_t* src = col + (piece << 4);
        const uint4 bv = gload16(bcol + (piece << 4));
        const uint32_t b[4] = {bv.x & 0x3f3f3f3fu, bv.y & 0x3f3f3f3fu, bv.z & 0x3f3f3f3fu, bv.w & 0x3f3f3f3fu};
        if (count_full) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int s = 0; s < 4; ++s) atomicAdd(&full[((b[q] >> (8 * s)) & 63u) * kECopies + copy], 1u);
            }
        }
        auto take = [&](const uint4& v, int slot) {
            const uint32_t w[4] = {v.x & 0x3f3f3f3fu, v.y & 0x3f3f3f3fu, v.z & 0x3f3f3f3fu, v.w & 0x3f3f3f3fu};
            uint32_t* mine = corr + (size_t)slot * 64 * copies + cp;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // bit 7 of each byte: leaf > base (128 + leaf - base - 1 stays within 64..190: no borrow between bytes)
                const uint32_t gt = ((w[q] | 0x80808080u) - b[q] - 0x01010101u) & 0x80808080u;
                if (gt) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((gt >> (8 * s + 7)) & 1u) {
                            atomicAdd(&mine[((w[q] >> (8 * s)) & 63u) * copies], 1u);
                            atomicAdd(&mine[((b[q] >> (8 * s)) & 63u) * copies], 0xFFFFFFFFu);
                        }
                }
            }
        };
        int j = 0;
        for (; j + kEUnroll <= ccount; j += kEUnroll) {
            uint4 v[kEUnroll];
#pragma unroll
            for (int u = 0; u < kEUnroll; ++u) v[u] = gload16(src + (size_t)rows[c0 + j + u] * row_stride);
#pragma unroll
            for (int u = 0; u < kEUnroll; ++u) take(v[u], j + u);
        }
        for (; j < ccount; ++j) take(gload16(src + (size_t)rows[c0 + j] * row_stride), j);
    }
    __syncthreads();
    if (count_full && threadIdx.x < 64) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kECopies; ++c) s += full[threadIdx.x * kECopies + ((c + threadIdx.x) & (kECopies - 1))];
        if (s) atomicAdd(&hist[((size_t)nrows * K + kk) * 64 + threadIdx.x], s);
    }
    for (int i = threadIdx.x; i < ccount * 64; i += blockDim.x) {
        uint32_t v = 0;
        for (int c = 0; c < copies; ++c) v += corr[(size_t)i * copies + c];
        if (v) atomicAdd(&hist[((size_t)(c0 + i / 64) * K + kk) * 64 + (i & 63)], v);
    }
}

// rows 0..nrows-1 hold corrections: add base's histogram (row nrows)
__global__ __launch_bounds__(256) void extend_finish_kernel(uint32_t* __restrict__ hist, int nrows, int K) {
    const size_t per = (size_t)K * 64, total = (size_t)nrows * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        hist[i] += hist[total + i % per];
}

// the empty base: hist[(r * K + kk) * 64 + bin] of leaf row rows[r] itself.  blockIdx.x = (r * K + kk) * tiles + tile, a
// workgroup takes four 16-byte pieces per thread
__global__ __launch_bounds__(1024) void rows_hist_kernel(const uint8_t* __restrict__ leaf, int K, int p,
                                                         const int32_t* __restrict__ rows, int tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[64 * kECopies];
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int r = blockIdx.x / tiles / K;
    for (int i = threadIdx.x; i < 64 * kECopies; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const size_t m16 = ((size_t)1 << p) >> 4;
    const uint8_t* src = leaf + (((size_t)rows[r] * K + kk) << p);
    const int copy = threadIdx.x & (kECopies - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t piece = ((size_t)tile * 4 + q) * blockDim.x + threadIdx.x;
        if (piece < m16) {
            const uint4 v = gload16(src + (piece << 4));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int s = 0; s < 4; ++s) atomicAdd(&h[((w[a] >> (8 * s)) & 63u) * kECopies + copy], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kECopies; ++c) s += h[threadIdx.x * kECopies + ((c + threadIdx.x) & (kECopies - 1))];
        if (s) atomicAdd(&hist[((size_t)r * K + kk) * 64 + threadIdx.x], s);
    }
}

__global__ __launch_bounds__(256) void extend_fold_kernel(uint8_t* __restrict__ base, const uint8_t* __restrict__ row, size_t len16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 a = gload16(base + (i << 4)), b = gload16(row + (i << 4));
        gstore16(base + (i << 4), make_uint4(bmax4(a.x, b.x), bmax4(a.y, b.y), bmax4(a.z, b.z), bmax4(a.w, b.w)));
    }
}

size_t extend_lds_bytes(int slots) { return sizeof(uint32_t) * (64 * kECopies + (size_t)slots * 64); }

}  // namespace

void launch_extend(const uint8_t* base_dev, const uint8_t* leaf_dev, int K, int p, const int32_t* rows_dev, int nrows,
                   uint32_t* hist_dev, hipStream_t st) {
    if (K <= 0 || nrows <= 0) return;
    const size_t m16 = ((size_t)1 << p) >> 4;
    (void)hipMemsetAsync(hist_dev, 0, (size_t)(nrows + 1) * K * 64 * sizeof(uint32_t), st);
    if (!base_dev) {
        const size_t t = m16 < 1024 ? (m16 < 64 ? 64 : m16) : 1024;
        const size_t tiles = (m16 + t * 4 - 1) / (t * 4);
        hipLaunchKernelGGL(rows_hist_kernel, dim3((unsigned)((size_t)nrows * K * tiles)), dim3((unsigned)t), 0, st, leaf_dev, K, p,
                           rows_dev, (int)tiles, hist_dev);
        return;
    }
    // copies: the largest power of two (<= 8) that keeps the corrections within kCopySlots rows of 64 (40 KiB + 8 KiB: three
    // workgroups per CU; copies that push a CU down to two cost the HBM-bound steps 5-10 %, profiles/greedy_extend.txt)
    int copies = 1;
    while (copies < 8 && nrows * copies * 2 <= kCopySlots) copies *= 2;
    const int per_tile = kTileC / copies;
    const int ctiles = (nrows + per_tile - 1) / per_tile;
    const int threads = (int)(m16 < (size_t)kEThreads ? (m16 < 64 ? 64 : m16) : kEThreads);
    // about four workgroups per CU over the whole grid (two resident at a time), never more than one piece per thread
    const size_t most = (m16 + threads - 1) / threads;
    size_t tiles = (1024 + (size_t)K * ctiles - 1) / ((size_t)K * ctiles);
    if (tiles > most) tiles = most;
    if (tiles < 1) tiles = 1;
    const int slots = (nrows < per_tile ? nrows : per_tile) * copies;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(extend_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)extend_lds_bytes(kTileC)) != hipSuccess)
            (void)hipGetLastError();
        attr = true;
    }
    hipLaunchKernelGGL(extend_kernel, dim3((unsigned)((size_t)ctiles * K * tiles)), dim3(threads), extend_lds_bytes(slots), st, base_dev,
                       leaf_dev, K, p, rows_dev, nrows, (int)tiles, copies, hist_dev);
    const size_t total = (size_t)nrows * K * 64;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(extend_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, hist_dev, nrows, K);
}

void launch_extend_fold(uint8_t* base_dev, const uint8_t* row_dev, size_t len, hipStream_t st) {
    const size_t len16 = len >> 4;
    if (!len16) return;
    size_t blocks = (len16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(extend_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, base_dev, row_dev, len16);
}

}  // namespace dd
