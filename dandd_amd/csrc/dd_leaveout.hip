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
// Histograms: the full union in LDS privatised 32 ways (dd_union.hip's image: h[bin][copy]); the corrections of up to
// kTileG = 256 groups as [group][64] u32 in LDS (64 KiB + 8 KiB: two workgroups per CU).  More groups (n up to 4096) are
// cut into group tiles of 256, one grid slice each, every slice reading the slab again and only tile 0 counting the full
// union.  A workgroup flushes once, one global atomic per non-zero bin, 64 contiguous bins per row; leaveout_finish_kernel
// adds the full union to every group row.  HBM-bound: the slab (n K m bytes) is read once per group tile.
#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

constexpr int kTileG = 256;      // groups whose corrections one workgroup keeps in LDS
constexpr int kLCopies = 32;     // privatised copies of the full-union histogram
constexpr int kLThreads = 512;
constexpr int kNotLast = -2;     // tab[2 j + 1] of a leaf that does not end its group
constexpr int kUnroll = 8;       // leaf rows in flight per thread

// grid: blockIdx.x = (gtile * K + kk) * tiles + tile; a workgroup takes every tiles-th 16-byte piece of k column kk
// tab[2 j] = leaf row of slot j, tab[2 j + 1] = its group when slot j is the last of its group (-1: the floor), else kNotLast
__global__ __launch_bounds__(kLThreads) void leaveout_kernel(const uint8_t* __restrict__ leaf, int K, int p,
                                                             const int32_t* __restrict__ tab, int nslots, int G, int tiles,
                                                             uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lds[];            // full[64][kLCopies], then corr[gcount][64]
    uint32_t* full = lds;
    uint32_t* corr = lds + 64 * kLCopies;
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int gtile = blockIdx.x / tiles / K;
    const int g0 = gtile * kTileG;
    const int gcount = G - g0 < kTileG ? G - g0 : kTileG;
    const bool count_full = gtile == 0;
    for (int i = threadIdx.x; i < 64 * kLCopies + gcount * 64; i += blockDim.x) lds[i] = 0;
    __syncthreads();

    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t row_stride = (size_t)K << p;    // bytes from one leaf's row kk to the next leaf's
    const uint8_t* col = leaf + ((size_t)kk << p);
    const int copy = threadIdx.x & (kLCopies - 1);
    for (size_t piece = (size_t)tile * blockDim.x + threadIdx.x; piece < m16; piece += (size_t)tiles * blockDim.x) {
        const uint8_t* src = col + (piece << 4);
        uint32_t b1[4] = {0, 0, 0, 0}, b2[4] = {0, 0, 0, 0}, fl[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
        int g1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) g1[r] = -1;
        auto take = [&](const uint4& v, int code) {
            const uint32_t w[4] = {v.x & 0x3f3f3f3fu, v.y & 0x3f3f3f3fu, v.z & 0x3f3f3f3fu, v.w & 0x3f3f3f3fu};
#pragma unroll
            for (int q = 0; q < 4; ++q) mx[q] = bmax4(mx[q], w[q]);
            if (code == kNotLast) return;
            if (code < 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) fl[q] = bmax4(fl[q], mx[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // bit 7 of each byte: M > b1 (128 + M - b1 - 1 stays within 64..190: no borrow between bytes)
                    const uint32_t gt = ((mx[q] | 0x80808080u) - b1[q] - 0x01010101u) & 0x80808080u;
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
                if (count_full) atomicAdd(&full[x1 * kLCopies + copy], 1u);
                const int gl = g1[4 * q + b] - g0;
                if (x2 < x1 && (unsigned)gl < (unsigned)gcount) {
                    atomicAdd(&corr[gl * 64 + x1], 0xFFFFFFFFu);
                    atomicAdd(&corr[gl * 64 + x2], 1u);
                }
            }
        }
    }
    __syncthreads();
    if (count_full && threadIdx.x < 64) {
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < kLCopies; ++c) s += full[threadIdx.x * kLCopies + ((c + threadIdx.x) & (kLCopies - 1))];
        if (s) atomicAdd(&hist[((size_t)G * K + kk) * 64 + threadIdx.x], s);
    }
    for (int i = threadIdx.x; i < gcount * 64; i += blockDim.x) {
        const uint32_t v = corr[i];
        if (v) atomicAdd(&hist[((size_t)(g0 + i / 64) * K + kk) * 64 + (i & 63)], v);
    }
}

// rows 0..G-1 hold corrections: add the full union (row G)
__global__ __launch_bounds__(256) void leaveout_finish_kernel(uint32_t* __restrict__ hist, int G, int K) {
    const size_t per = (size_t)K * 64, total = (size_t)G * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        hist[i] += hist[total + i % per];
}

}  // namespace

static size_t leaveout_lds_bytes(int G) {
    const int gcount = G < kTileG ? G : kTileG;
    return sizeof(uint32_t) * (64 * kLCopies + (size_t)gcount * 64);
}

void launch_leaveout(const uint8_t* leaf_dev, int K, int p, const int32_t* tab_dev, int nslots, int G, uint32_t* hist_dev,
                     hipStream_t st) {
    if (K <= 0 || G <= 0 || nslots <= 0) return;
    const size_t m16 = ((size_t)1 << p) >> 4;
    const int threads = (int)(m16 < (size_t)kLThreads ? (m16 < 64 ? 64 : m16) : kLThreads);
    const int gtiles = (G + kTileG - 1) / kTileG;
    // about four workgroups per CU over the whole grid (two resident at a time), never more than one piece per thread
    const size_t most = (m16 + threads - 1) / threads;
    size_t tiles = (1024 + (size_t)K * gtiles - 1) / ((size_t)K * gtiles);
    if (tiles > most) tiles = most;
    if (tiles < 1) tiles = 1;
    const size_t lds = leaveout_lds_bytes(G);
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(leaveout_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)leaveout_lds_bytes(kTileG)) != hipSuccess)
            (void)hipGetLastError();
        attr = true;
    }
    (void)hipMemsetAsync(hist_dev, 0, (size_t)(G + 1) * K * 64 * sizeof(uint32_t), st);
    hipLaunchKernelGGL(leaveout_kernel, dim3((unsigned)((size_t)gtiles * K * tiles)), dim3(threads), lds, st, leaf_dev, K, p,
                       tab_dev, nslots, G, (int)tiles, hist_dev);
    const size_t total = (size_t)G * K * 64;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(leaveout_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, hist_dev, G, K);
}

}  // namespace dd
