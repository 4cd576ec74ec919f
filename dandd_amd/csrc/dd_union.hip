// dd_union.hip -- K2 (byte-max union + 64-bin register histograms) and K3 (Ertl MLE on device).
//
// Replaces  dashing union -z -o <out> <in...>   (/root/reference/lib/sketch_classes.py:368-373)
// and the histogram half of  dashing card --presketched <path>  (:306-321), batched over the
// union schedules DandD generates:
//   * N-way union                      (DeltaTree root / any tree node)
//   * running max along an ordering     (DeltaTree.sketch_ordering, lib/huffman_dandd.py:644-663;
//                                        equals the flat prefix unions because max is associative)
//   * all pairs                         (DeltaTree.pairwise_spiders, lib/huffman_dandd.py:666-695)
// HBM/L2-bound: 16-byte loads, SWAR byte max, LDS histograms privatised 32 ways, bin-major (one bank per copy).
#include "dd_k2.h"
#include "dd_kernels.h"

namespace dd {
namespace {

__global__ __launch_bounds__(256) void union_kernel(const uint8_t* const* __restrict__ in, int n,
                                                    size_t len16, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len16;
         i += (size_t)gridDim.x * blockDim.x) {
        uint4 acc = reinterpret_cast<const uint4*>(in[0])[i];
        for (int j = 1; j < n; ++j) acc = bmax16(acc, reinterpret_cast<const uint4*>(in[j])[i]);
        reinterpret_cast<uint4*>(out)[i] = acc;
    }
}

// PC = 16-byte pieces per thread: a workgroup's tile is PC x 16 KiB of a row.  Rows of 64 KiB and more use PC = 4:
// four times fewer barriers, histogram folds and (rows of several tiles add their partial histograms with global
// atomics) global atomics per byte -- 264 M of those for the pairs of 64 sketches of 1 MiB before.
// one workgroup per (job, tile of its registers): job's row is row `job` of regs, or with a row list (job = r * K + kk)
// column kk of leaf rows[r]
template <int PC>
__global__ __launch_bounds__(1024) void hist_kernel(const uint8_t* __restrict__ regs, int p, int tiles,
                                                    const int32_t* __restrict__ rows, int K,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kHistWords];
    const int job = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const size_t row = rows ? (size_t)rows[job / K] * K + job % K : (size_t)job;
    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t piece = (size_t)tile * blockDim.x * PC + threadIdx.x;
    hist_zero(h);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PC; ++q)
        if (piece + (size_t)q * blockDim.x < m16)
            hist_add16(h, reinterpret_cast<const uint4*>(regs + (row << p))[piece + (size_t)q * blockDim.x]);
    __syncthreads();
    hist_flush(h, hist + (size_t)job * 64, tiles == 1);
}

// one workgroup per (ordering, k, tile): running max over the ordering, one histogram per prefix
template <int PC>
__global__ __launch_bounds__(1024) void progressive_kernel(const uint8_t* __restrict__ leaf, int n,
                                                           int K, int p, int tiles,
                                                           const int32_t* __restrict__ ord,
                                                           uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kHistWords];
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int o = blockIdx.x / tiles / K;
    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t piece = (size_t)tile * blockDim.x * PC + threadIdx.x;
    uint4 run[PC];
#pragma unroll
    for (int q = 0; q < PC; ++q) run[q] = make_uint4(0, 0, 0, 0);
    for (int j = 0; j < n; ++j) {
        const int gi = ord[(size_t)o * n + j];
        hist_zero(h);
        __syncthreads();
        const uint8_t* src = leaf + (((size_t)gi * K + kk) << p);
#pragma unroll
        for (int q = 0; q < PC; ++q)
            if (piece + (size_t)q * blockDim.x < m16) {
                run[q] = bmax16(run[q], reinterpret_cast<const uint4*>(src)[piece + (size_t)q * blockDim.x]);
                hist_add16(h, run[q]);
            }
        __syncthreads();
        hist_flush(h, hist + (((size_t)o * n + j) * K + kk) * 64, tiles == 1);
        __syncthreads();
    }
}

// one workgroup per (i, k, tile): row i of the pair matrix, j = i..n-1
template <int PC>
__global__ __launch_bounds__(1024) void pairwise_kernel(const uint8_t* __restrict__ leaf, int n,
                                                        int K, int p, int tiles,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kHistWords];
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int i = blockIdx.x / tiles / K;
    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t piece = (size_t)tile * blockDim.x * PC + threadIdx.x;
    uint4 a[PC];
#pragma unroll
    for (int q = 0; q < PC; ++q) {
        a[q] = make_uint4(0, 0, 0, 0);
        if (piece + (size_t)q * blockDim.x < m16)
            a[q] = reinterpret_cast<const uint4*>(leaf + (((size_t)i * K + kk) << p))[piece + (size_t)q * blockDim.x];
    }
    for (int j = i; j < n; ++j) {
        hist_zero(h);
        __syncthreads();
        const uint8_t* src = leaf + (((size_t)j * K + kk) << p);
#pragma unroll
        for (int q = 0; q < PC; ++q)
            if (piece + (size_t)q * blockDim.x < m16)
                hist_add16(h, bmax16(a[q], reinterpret_cast<const uint4*>(src)[piece + (size_t)q * blockDim.x]));
        __syncthreads();
        hist_flush(h, hist + (((size_t)i * n + j) * K + kk) * 64, tiles == 1);
        __syncthreads();
    }
}

// the rectangle (dd_cross): one workgroup per (s, k, tile) -- row s of slab a against every row j of slab b
template <int PC>
__global__ __launch_bounds__(1024) void cross_stream_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int nb,
                                                            int K, int p, int tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kHistWords];
    const int tile = blockIdx.x % tiles;
    const int kk = (blockIdx.x / tiles) % K;
    const int s = blockIdx.x / tiles / K;
    const size_t m16 = ((size_t)1 << p) >> 4;
    const size_t piece = (size_t)tile * blockDim.x * PC + threadIdx.x;
    uint4 mine[PC];
#pragma unroll
    for (int q = 0; q < PC; ++q) {
        mine[q] = make_uint4(0, 0, 0, 0);
        if (piece + (size_t)q * blockDim.x < m16)
            mine[q] = reinterpret_cast<const uint4*>(a + (((size_t)s * K + kk) << p))[piece + (size_t)q * blockDim.x];
    }
    for (int j = 0; j < nb; ++j) {
        hist_zero(h);
        __syncthreads();
        const uint8_t* src = b + (((size_t)j * K + kk) << p);
#pragma unroll
        for (int q = 0; q < PC; ++q)
            if (piece + (size_t)q * blockDim.x < m16)
                hist_add16(h, bmax16(mine[q], reinterpret_cast<const uint4*>(src)[piece + (size_t)q * blockDim.x]));
        __syncthreads();
        hist_flush(h, hist + (((size_t)s * nb + j) * K + kk) * 64, tiles == 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mle_kernel(const uint32_t* __restrict__ hist, size_t njobs,
                                                  int p, double relerr, double* __restrict__ est) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    uint32_t c[64];
    uint64_t tot = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        c[i] = hist[j * 64 + i];
        tot += c[i];
    }
    // a histogram that does not count exactly m registers is an unused slot (e.g. the lower
    // triangle of the pair matrix): report 0 instead of walking off the array
    est[j] = (tot == (1ull << p)) ? ertl_mle(c, p, relerr) : 0.0;
}

inline int pieces_for(int p) { return p >= 16 ? 4 : 1; }  // 16-byte pieces per thread (the kernels' PC)
inline int tiles_for(int p) {
    const size_t m16 = ((size_t)1 << p) >> 4, per_tile = (size_t)1024 * pieces_for(p);
    return (int)((m16 + per_tile - 1) / per_tile);
}
inline int threads_for(int p) {
    const size_t m16 = ((size_t)1 << p) >> 4;
    size_t t = m16 < 1024 ? m16 : 1024;
    if (t < 64) t = 64;
    return (int)t;
}
// one of a kernel's two PC forms, by the row size: a workgroup per (job, tile)
template <typename Kernel, typename... Args>
void launch_pc(Kernel pc4, Kernel pc1, int p, size_t jobs, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(pieces_for(p) == 4 ? pc4 : pc1, dim3((unsigned)(jobs * tiles_for(p))), dim3(threads_for(p)), 0, st, args...);
}

}  // namespace

void launch_union(const uint8_t* const* in_dev, int n, size_t len, uint8_t* out_dev, hipStream_t st) {
    const size_t len16 = len >> 4;
    if (!len16) return;
    size_t blocks = (len16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(union_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in_dev, n, len16, out_dev);
}

void launch_hist(const uint8_t* regs_dev, int njobs, int p, uint32_t* hist_dev, hipStream_t st) {
    if (njobs <= 0) return;
    if (tiles_for(p) > 1) (void)hipMemsetAsync(hist_dev, 0, (size_t)njobs * 64 * sizeof(uint32_t), st);
    launch_pc(hist_kernel<4>, hist_kernel<1>, p, njobs, st, regs_dev, p, tiles_for(p), (const int32_t*)nullptr, 1, hist_dev);
}

void launch_rows_hist(const uint8_t* leaf_dev, int K, int p, const int32_t* rows_dev, int nrows, uint32_t* hist_dev, hipStream_t st) {
    if (K <= 0 || nrows <= 0) return;
    launch_pc(hist_kernel<4>, hist_kernel<1>, p, (size_t)nrows * K, st, leaf_dev, p, tiles_for(p), rows_dev, K, hist_dev);
}

void launch_progressive(const uint8_t* leaf_dev, int n, int K, int p, const int32_t* ord_dev,
                        int norder, uint32_t* hist_dev, hipStream_t st) {
    if (n <= 0 || K <= 0 || norder <= 0) return;
    if (tiles_for(p) > 1) (void)hipMemsetAsync(hist_dev, 0, (size_t)norder * n * K * 64 * sizeof(uint32_t), st);
    launch_pc(progressive_kernel<4>, progressive_kernel<1>, p, (size_t)norder * K, st, leaf_dev, n, K, p, tiles_for(p), ord_dev, hist_dev);
}

void launch_pairwise(const uint8_t* leaf_dev, int n, int K, int p, uint32_t* hist_dev, hipStream_t st) {
    if (n <= 0 || K <= 0) return;
    (void)hipMemsetAsync(hist_dev, 0, (size_t)n * n * K * 64 * sizeof(uint32_t), st);
    launch_pc(pairwise_kernel<4>, pairwise_kernel<1>, p, (size_t)n * K, st, leaf_dev, n, K, p, tiles_for(p), hist_dev);
}

void launch_cross_stream(const uint8_t* a_dev, int na, const uint8_t* b_dev, int nb, int K, int p, uint32_t* hist_dev, hipStream_t st) {
    if (na <= 0 || nb <= 0 || K <= 0) return;
    if (tiles_for(p) > 1) (void)hipMemsetAsync(hist_dev, 0, (size_t)na * nb * K * 64 * sizeof(uint32_t), st);
    launch_pc(cross_stream_kernel<4>, cross_stream_kernel<1>, p, (size_t)na * K, st, a_dev, b_dev, nb, K, p, tiles_for(p), hist_dev);
}

void launch_mle(const uint32_t* hist_dev, size_t njobs, int p, double* est_dev, hipStream_t st) {
    if (!njobs) return;
    hipLaunchKernelGGL(mle_kernel, dim3((unsigned)((njobs + 255) / 256)), dim3(256), 0, st, hist_dev,
                       njobs, p, mle_relerr(p), est_dev);
}

}  // namespace dd
