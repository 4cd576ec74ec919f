// dd_leaveout.hip -- K2 leave-out unions: the register histogram of every "union of all leaves but group g" from ONE read
// of the leaf slab.
//
// Replaces, for `dandd deltadelta` (DeltaTree.find_delta_delta, the reference's lib/huffman_dandd.py:559-566), one
// (n-1)-way `dashing union` + `dashing card` per left-out group and climb step: what is needed per (group, k) is the 64-bin
// histogram of the byte-max over every leaf outside the group.
//
// Top two by group.  At one register let b1 be the largest value over all groups, g1 a group that holds it and b2 the
// largest value over the groups other than g1.  The union of every leaf outside group g then holds b1 at that register --
// unless g is the ONLY group that holds b1 (g = g1 and b2 < b1), where it holds b2.  So
//         hist_rest(g) = hist_all + corr_g,    corr_g[b1] -= 1, corr_g[b2] += 1  for every register where g alone holds b1,
// exact integers (u32 arithmetic mod 2^32: a bin of corr_g never goes below -hist_all[bin]).  A tie between two groups
// leaves b2 = b1: no correction.  Leaves of group -1 (always in every union, never left out) only raise a floor f:
// b1' = max(b1, f), b2' = max(b2, f), and a correction is made only where b2' < b1'.
//
// The host orders the leaves by group (the floor first) and marks the last leaf of each group, so the kernel folds one
// group maximum M at a time and a group never meets itself: if M > b1 { b2 = b1; b1 = M; g1 = g } else b2 = max(b2, M).
// Four registers per dword (SWAR byte max, bytes <= 63), sixteen per thread per 16-byte load; the group ids of the
// sixteen registers stay in VGPRs.
//
// Histograms: the full union in LDS privatised 32 ways (dd_k2.h's image: h[bin][copy]); the corrections of up to
// kCorrTile = 256 groups as [group][64] u32 in LDS (64 KiB + 8 KiB: two workgroups per CU).  More groups (n up to 4096) are
// cut into group tiles of 256, one grid slice each, every slice reading the slab again and only tile 0 counting the full
// union.  A workgroup flushes once, one global atomic per non-zero bin, 64 contiguous bins per row; corr_finish_kernel
// adds the full union to every group row.  HBM-bound: the slab (n K m bytes) is read once per group tile.
#include "dd_k2.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kNotLast = -2;     // tab[2 j + 1] of a leaf that does not end its group
constexpr int kUnroll = 8;       // leaf rows in flight per thread

// grid: blockIdx.x = (gtile * K + kk) * tiles + tile; a workgroup takes every tiles-th 16-byte piece of k column kk
// tab[2 j] = leaf row of slot j, tab[2 j + 1] = its group when slot j is the last of its group (-1: the floor), else kNotLast
__global__ __launch_bounds__(kCorrThreads) void leaveout_kernel(const uint8_t* __restrict__ leaf, int K, int p,
                                                                const int32_t* __restrict__ tab, int nslots, int G, int tiles,
                                                                uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lds[];            // the image of the full union, then corr[gcount][64]
    uint32_t* corr = corr_of(lds);
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int gtile = blockIdx.x / tiles / K;
    const int g0 = gtile * kCorrTile;
    const int gcount = G - g0 < kCorrTile ? G - g0 : kCorrTile;
    const bool count_full = gtile == 0;
    corr_zero(lds, gcount);
    __syncthreads();

    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t row_stride = (size_t)K << p;    // bytes from one leaf's row kk to the next leaf's
    const uint8_t* col = leaf + ((size_t)kk << p);
    for (size_t piece = (size_t)tile * blockDim.x + threadIdx.x; piece < m16; piece += (size_t)tiles * blockDim.x) {
        const uint8_t* src = col + (piece << 4);
        uint32_t b1[4] = {0, 0, 0, 0}, b2[4] = {0, 0, 0, 0}, fl[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
        int g1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) g1[r] = -1;
        auto take = [&](const uint4& v, int code) {
            uint32_t w[4];
            unpack16(v, w);
#pragma unroll
            for (int q = 0; q < 4; ++q) mx[q] = bmax4(mx[q], w[q]);
            if (code == kNotLast) return;
            if (code < 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) fl[q] = bmax4(fl[q], mx[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t gt = bgt4(mx[q], b1[q]);   // bit 7 of each byte: M > b1
                    const uint32_t mk = (gt >> 7) * 0xFFu;
                    b2[q] = (b1[q] & mk) | (bmax4(b2[q], mx[q]) & ~mk);
                    b1[q] = bmax4(b1[q], mx[q]);
#pragma unroll
                    for (int b = 0; b < 4; ++b) g1[4 * q + b] = ((gt >> (8 * b + 7)) & 1u) ? code : g1[4 * q + b];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) mx[q] = 0;
        };
        int j = 0;
        for (; j + kUnroll <= nslots; j += kUnroll) {
            uint4 v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) v[u] = gload16(src + (size_t)tab[2 * (j + u)] * row_stride);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) take(v[u], tab[2 * (j + u) + 1]);
        }
        for (; j < nslots; ++j) take(gload16(src + (size_t)tab[2 * j] * row_stride), tab[2 * j + 1]);

#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t u1 = bmax4(b1[q], fl[q]), u2 = bmax4(b2[q], fl[q]);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t x1 = (u1 >> (8 * b)) & 63u, x2 = (u2 >> (8 * b)) & 63u;
                if (count_full) hist_add(lds, x1);
                const int gl = g1[4 * q + b] - g0;
                if (x2 < x1 && (unsigned)gl < (unsigned)gcount) {
                    atomicAdd(&corr[gl * 64 + x1], 0xFFFFFFFFu);
                    atomicAdd(&corr[gl * 64 + x2], 1u);
                }
            }
        }
    }
    __syncthreads();
    corr_flush(lds, count_full, g0, gcount, 1, G, K, kk, hist);
}

// rows 0..nrows-1 hold corrections: add row nrows (leave-out: the full union; extend: base's own histogram)
__global__ __launch_bounds__(256) void corr_finish_kernel(uint32_t* __restrict__ hist, int nrows, int K) {
    const size_t per = (size_t)K * 64, total = (size_t)nrows * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        hist[i] += hist[total + i % per];
}

}  // namespace

void launch_corr_finish(uint32_t* hist_dev, int nrows, int K, hipStream_t st) {
    const size_t total = (size_t)nrows * K * 64;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(corr_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, hist_dev, nrows, K);
}

void launch_leaveout(const uint8_t* leaf_dev, int K, int p, const int32_t* tab_dev, int nslots, int G, uint32_t* hist_dev,
                     hipStream_t st) {
    if (K <= 0 || G <= 0 || nslots <= 0) return;
    const int gtiles = (G + kCorrTile - 1) / kCorrTile;
    const CorrShape sh = corr_shape(p, K, gtiles);
    (void)hipMemsetAsync(hist_dev, 0, (size_t)(G + 1) * K * 64 * sizeof(uint32_t), st);
    launch_full_lds<leaveout_kernel>(dim3((unsigned)((size_t)gtiles * K * sh.tiles)), dim3(sh.threads),
                                     corr_lds_bytes(G < kCorrTile ? G : kCorrTile), st, leaf_dev, K, p,
                                     tab_dev, nslots, G, sh.tiles, hist_dev);
    launch_corr_finish(hist_dev, G, K, st);
}

}  // namespace dd
