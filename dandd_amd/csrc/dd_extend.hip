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
// borrow trick of leaveout_kernel (bgt4, bytes <= 63).  hist(base) itself is counted by candidate tile 0 in an LDS image
// privatised 32 ways (dd_k2.h's: h[bin][copy]).
//
// The corrections of up to kCorrTile = 256 candidates sit in LDS as corr[candidate][64][copies] u32 (64 KiB + 8 KiB: two
// workgroups per CU); with fewer candidates some of the room goes to `copies` (a power of two, copy = lane % copies),
// which cuts the lanes that meet on one word when base is small and most registers correct -- the first steps of a walk
// over unrelated genomes, the only ones that are LDS-atomic-bound (profiles/greedy_extend.txt).  More candidates are cut into tiles of 256, one grid slice each.  A workgroup flushes once, one
// global atomic per non-zero bin; corr_finish_kernel adds hist(base) to every candidate row.
//
// An EMPTY base needs no corrections at all (every non-zero register would be one): dd_union.hip's hist_kernel counts the
// listed rows' own histograms.
#include "dd_k2.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kCopySlots = 160;  // the rows of 64 corrections that `copies` may widen the candidates' to
constexpr int kEUnroll = 8;      // candidate rows in flight per thread

// grid: blockIdx.x = (ctile * K + kk) * tiles + tile; a workgroup takes every tiles-th 16-byte piece of k column kk
// hist[(r * K + kk) * 64 + bin]: corrections of candidate slot r < nrows; row nrows: base's own histogram
__global__ __launch_bounds__(kCorrThreads) void extend_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ leaf,
                                                           int K, int p, const int32_t* __restrict__ rows, int nrows, int tiles,
                                                           int copies, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lds[];            // the image of base, then corr[ccount][64][copies]
    uint32_t* corr = corr_of(lds);
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int ctile = blockIdx.x / tiles / K;
    const int per_tile = kCorrTile / copies;
    const int c0 = ctile * per_tile;
    const int ccount = nrows - c0 < per_tile ? nrows - c0 : per_tile;
    const bool count_full = ctile == 0;
    corr_zero(lds, ccount * copies);
    __syncthreads();

    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t row_stride = (size_t)K << p;    // bytes from one leaf's row kk to the next leaf's
    const uint8_t* col = leaf + ((size_t)kk << p);
    const uint8_t* bcol = base + ((size_t)kk << p);
    const int cp = threadIdx.x & (copies - 1);
    for (size_t piece = (size_t)tile * blockDim.x + threadIdx.x; piece < m16; piece += (size_t)tiles * blockDim.x) {
        const uint8_t* src = col + (piece << 4);
        const uint4 bv = gload16(bcol + (piece << 4));
        uint32_t b[4];
        unpack16(bv, b);
        if (count_full) hist_add16(lds, b);
        auto take = [&](const uint4& v, int slot) {
            uint32_t w[4];
            unpack16(v, w);
            uint32_t* mine = corr + (size_t)slot * 64 * copies + cp;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t gt = bgt4(w[q], b[q]);   // bit 7 of each byte: leaf > base
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
    corr_flush(lds, count_full, c0, ccount, copies, nrows, K, kk, hist);
}

__global__ __launch_bounds__(256) void extend_fold_kernel(uint8_t* __restrict__ base, const uint8_t* __restrict__ row, size_t len16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len16; i += (size_t)gridDim.x * blockDim.x) {
        gstore16(base + (i << 4), bmax16(gload16(base + (i << 4)), gload16(row + (i << 4))));
    }
}

}  // namespace

void launch_extend(const uint8_t* base_dev, const uint8_t* leaf_dev, int K, int p, const int32_t* rows_dev, int nrows,
                   uint32_t* hist_dev, hipStream_t st) {
    if (K <= 0 || nrows <= 0) return;
    (void)hipMemsetAsync(hist_dev, 0, (size_t)(nrows + 1) * K * 64 * sizeof(uint32_t), st);
    if (!base_dev) {
        launch_rows_hist(leaf_dev, K, p, rows_dev, nrows, hist_dev, st);
        return;
    }
    // copies: the largest power of two (<= 8) that keeps the corrections within kCopySlots rows of 64 (40 KiB + 8 KiB: three
    // workgroups per CU; copies that push a CU down to two cost the HBM-bound steps 5-10 %, profiles/greedy_extend.txt)
    int copies = 1;
    while (copies < 8 && nrows * copies * 2 <= kCopySlots) copies *= 2;
    const int per_tile = kCorrTile / copies;
    const int ctiles = (nrows + per_tile - 1) / per_tile;
    const CorrShape sh = corr_shape(p, K, ctiles);
    launch_full_lds<extend_kernel>(dim3((unsigned)((size_t)ctiles * K * sh.tiles)), dim3(sh.threads),
                                   corr_lds_bytes((nrows < per_tile ? nrows : per_tile) * copies), st, base_dev, leaf_dev, K, p,
                                   rows_dev, nrows, sh.tiles, copies, hist_dev);
    launch_corr_finish(hist_dev, nrows, K, st);
}

void launch_extend_fold(uint8_t* base_dev, const uint8_t* row_dev, size_t len, hipStream_t st) {
    const size_t len16 = len >> 4;
    if (!len16) return;
    size_t blocks = (len16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(extend_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, base_dev, row_dev, len16);
}

}  // namespace dd
