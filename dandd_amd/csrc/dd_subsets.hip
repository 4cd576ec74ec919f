// dd_subsets.hip -- K2 all-subset unions: the register histogram of the union of EVERY subset of n <= 16 leaves.
//
// For `dandd abba` (DeltaTree.ordering_expectations): every prefix of every ordering of n genomes is a subset, so the
// 2^n subset unions give the exact expectations over all n! orderings.  What is needed per (subset s, k) is the 64-bin
// histogram of max_{g in s} leaf_g.
//
// Counted as dd_pscan.hip counts prefixes: with the threshold bit planes B_g,v = { r : leaf_g[r] <= v },
//         F_s(v) = |{ r : max_{g in s} leaf_g[r] <= v }| = popcount(AND_{g in s} B_g,v),   hist_s(v) = F_s(v) - F_s(v-1),
// F_s = 0 below the column's smallest register vmin and m from its largest, vmax, on (gram_range_kernel of dd_gram.hip).
//
// Lattice scan.  s = (h, l): l the subset of the low six leaves, h the subset of the others.  Per plane word and
// threshold, lane l forms Lo_l = AND of its low leaves' words and lane j forms Hi_h (h = chunk * HC + j) of its high
// leaves' words -- every lane reads the same LDS words (broadcast reads).  Then for every h of the chunk Hi_h moves to a
// scalar register (v_readlane) and each (h, l) costs one v_and and one v_bcnt_u32_b32 into a counter held in a VGPR:
// three VALU instructions per 64 subsets, plane word and threshold.  A wave is one job (threshold t, chunk of HC h's);
// a workgroup's eight waves share the planes one convert stage (dd_k2.h's bit_slice) makes per tile of D plane
// words.  The counts stay in the lanes across every tile of the workgroup's register range and are written once to a
// scratch slice of their own (no atomics); subsets_finish_kernel sums the ranges and differences F into histograms.
// Exact integers throughout.
#include "dd_k2.h"
#include "dd_kernels.h"

#include <algorithm>

namespace dd {
namespace {

constexpr int SS_WAVES = 8;
constexpr int SS_THREADS = 64 * SS_WAVES;
constexpr int SS_NMAX = 16;       // leaves
constexpr int SS_LOW = 6;         // leaves whose subsets are spread over the lanes
constexpr int SS_DMAX = 64;       // plane words per tile

// wg[3 b .. 3 b + 2] = (k column, first job, offset of the column's first threshold in part) of workgroup b;
// blockIdx.y = register range.  Job j of column k: threshold j / nchunks, h chunk j % nchunks.
// part[((toff + t) * RR + rr) << n | s] = |{ r in range rr : max_{g in s} leaf_g[r] <= vmin + t }|
template <int HC>
__global__ __launch_bounds__(SS_THREADS) void subsets_kernel(const uint8_t* __restrict__ leaf, int n, int K, int p,
                                                             const uint32_t* __restrict__ rng, const int32_t* __restrict__ wg,
                                                             int nchunks, int D, int tiles, uint32_t* __restrict__ part) {
    extern __shared__ uint32_t lds[];            // planes [g][t - t0][DP]
    const int k = wg[3 * blockIdx.x], j0 = wg[3 * blockIdx.x + 1], toff = wg[3 * blockIdx.x + 2];
    const int rr = blockIdx.y, RR = gridDim.y;
    const int vmin = (int)rng[2 * k], vmax = (int)rng[2 * k + 1];
    const int T = vmax - vmin;                   // (the host gives a column with T = 0 no workgroup)
    const int jend = min(j0 + SS_WAVES, T * nchunks);
    const int t0 = j0 / nchunks, t1 = (jend - 1) / nchunks + 1;
    const int Tw = t1 - t0;
    const int DP = D < 4 ? 4 : D;                // rows of whole 16-byte groups; pad words stay 0 (counted by no subset but the empty one)
    if (D < 4) {
        for (int i = threadIdx.x; i < n * Tw * DP; i += SS_THREADS) lds[i] = 0;
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = j0 + wave;
    const bool active = job < jend;
    const int t = active ? job / nchunks : t0, c = active ? job % nchunks : 0;
    // sel[g] = 0 where leaf g is in this lane's part of the subset (low leaves: l = lane; high: h = c HC + lane), else ~0
    uint32_t sel[SS_NMAX];
    const uint32_t h = (uint32_t)(c * HC + lane);
#pragma unroll
    for (int g = 0; g < SS_NMAX; ++g)
        sel[g] = (g < SS_LOW ? (lane >> g) & 1 : (h >> (g - SS_LOW)) & 1) ? 0u : ~0u;
    uint32_t cnt[HC];
#pragma unroll
    for (int i = 0; i < HC; ++i) cnt[i] = 0;
    const size_t col = (size_t)k << p;
    const size_t row_stride = (size_t)K << p;
    const size_t word0 = (size_t)rr * D * tiles;
    const int units = n * D;
    const int va = vmin + t0, vb = vmin + t1;
    for (int tile = 0; tile < tiles; ++tile) {
        // ---- convert: (leaf, 32 registers) -> the words of thresholds va .. vb - 1
        for (int u = threadIdx.x; u < units; u += SS_THREADS) {
            const int g = u / D, d = u % D;
            const uint8_t* src = leaf + (size_t)g * row_stride + col + (word0 + (size_t)tile * D + d) * 32;
            const uint4 a = gload16(src);
            // (log2m 4: a column of 16 registers; the other half of the word gets 63, which is <= no threshold)
            const uint4 b = p >= 5 ? gload16(src + 16) : make_uint4(0x3f3f3f3fu, 0x3f3f3f3fu, 0x3f3f3f3fu, 0x3f3f3f3fu);
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t x[6];
            bit_slice(w, x);
            uint32_t* dst = lds + (size_t)g * Tw * DP + d;
            // le(v) = OR of eq(u) for u <= v, eq(u) = AND_q (x[q] ^ (bit q of u clear ? ~0 : 0)).  A rolled loop over the
            // (block-uniform) thresholds: the unrolled 64-way form kept a branch condition per threshold in scalar registers
            // and spilled them.
            uint32_t le = 0;
            for (int v = vmin; v < vb; ++v) {
                uint32_t eq = ~0u;
#pragma unroll
                for (int q = 0; q < 6; ++q) eq &= x[q] ^ (((v >> q) & 1) ? 0u : ~0u);
                le |= eq;
                if (v >= va) {
                    *dst = le;
                    dst += DP;
                }
            }
        }
        __syncthreads();
        // ---- scan
        if (active) {
            const uint4* rowp = reinterpret_cast<const uint4*>(lds + (size_t)(t - t0) * DP);
            const int rowq = Tw * DP / 4;            // 16-byte groups from one leaf's row to the next's
            for (int d4 = 0; d4 < DP / 4; ++d4) {
                uint32_t lo[4] = {~0u, ~0u, ~0u, ~0u}, hi[4] = {~0u, ~0u, ~0u, ~0u};
#pragma unroll
                for (int g = 0; g < SS_NMAX; ++g) {
                    if (g < n) {
                        const uint4 xv = rowp[(size_t)g * rowq + d4];
                        const uint32_t xs[4] = {xv.x | sel[g], xv.y | sel[g], xv.z | sel[g], xv.w | sel[g]};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (g < SS_LOW) lo[i] &= xs[i];
                            else hi[i] &= xs[i];
                        }
                    }
                }
                // (eight readlanes into eight scalars, then their ANDs and counts: one scalar reused by every readlane made
                // each count wait a cycle for the scalar its readlane had just written)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j0 = 0; j0 < HC; j0 += 8) {
                        constexpr int B = HC < 8 ? HC : 8;
                        uint32_t sv[B];
#pragma unroll
                        for (int j = 0; j < B; ++j) sv[j] = (uint32_t)__builtin_amdgcn_readlane((int)hi[i], j0 + j);
#pragma unroll
                        for (int j = 0; j < B; ++j) cnt[j0 + j] += __builtin_popcount(lo[i] & sv[j]);
                    }
                }
            }
        }
        __syncthreads();
    }
    const int L = n < SS_LOW ? n : SS_LOW;
    if (active && lane < (1 << L)) {
        uint32_t* out = part + (((size_t)(toff + t) * RR + rr) << n);
#pragma unroll
        for (int j = 0; j < HC; ++j) {
            const size_t hh = (size_t)c * HC + j;
            if ((hh << L) < ((size_t)1 << n)) gstore4(out + ((hh << L) | (size_t)lane), cnt[j]);
        }
    }
}

// one thread per (subset s, column kk of the chunk), s fastest: F over the thresholds (the sum of the ranges' counts),
// then hist[(s * Kc + kk) * 64 + v] = F(v) - F(v - 1).  The empty set gets m in bin 0 (estimate 0).
__global__ __launch_bounds__(256) void subsets_finish_kernel(const uint32_t* __restrict__ part, int n, int p, int k0, int Kc,
                                                             const uint32_t* __restrict__ rng, int RR, uint32_t* __restrict__ hist) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ((size_t)Kc << n)) return;
    const size_t s = idx & (((size_t)1 << n) - 1);
    const int kk = (int)(idx >> n);
    int toff = 0;
    for (int q = 0; q < kk; ++q) toff += (int)rng[2 * (k0 + q) + 1] - (int)rng[2 * (k0 + q)];
    const int vmin = (int)rng[2 * (k0 + kk)], vmax = (int)rng[2 * (k0 + kk) + 1];
    const uint32_t m = 1u << p;
    uint32_t* out = hist + ((size_t)s * Kc + kk) * 64;
    uint32_t prev = 0;
#pragma unroll
    for (int v4 = 0; v4 < 16; ++v4) {
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = 4 * v4 + i;
            uint32_t F;
            if (s == 0) F = m;
            else if (v < vmin) F = 0;
            else if (v >= vmax) F = m;
            else {
                F = 0;
                const uint32_t* src = part + (((size_t)(toff + v - vmin) * RR) << n) + s;
                for (int r = 0; r < RR; ++r) F += gload4(src + ((size_t)r << n));
            }
            o[i] = F - prev;
            prev = F;
        }
        gstore16(out + 4 * v4, make_uint4(o[0], o[1], o[2], o[3]));
    }
}

}  // namespace

// h values a wave takes at once: every high subset up to 64
static int subsets_hc(int n) { return n <= SS_LOW ? 1 : std::min(64, 1 << (n - SS_LOW)); }

SubsetsPlan plan_subsets(int n, int p, const uint32_t* rng_host, int k0, int Kc, size_t part_budget) {
    SubsetsPlan pl;
    pl.HC = subsets_hc(n);
    pl.nchunks = n <= SS_LOW ? 1 : (1 << (n - SS_LOW)) / pl.HC;
    size_t tsum = 0, base = 0;
    for (int kk = 0; kk < Kc; ++kk) {
        const int k = k0 + kk;
        const int T = (int)rng_host[2 * k + 1] - (int)rng_host[2 * k];
        const int jobs = T * pl.nchunks;
        for (int j = 0; j < jobs; j += SS_WAVES) {
            pl.wg.push_back(k);
            pl.wg.push_back(j);
            pl.wg.push_back((int32_t)tsum);
        }
        tsum += (size_t)T;
        base += (size_t)(jobs + SS_WAVES - 1) / SS_WAVES;
    }
    const size_t words = std::max<size_t>(1, ((size_t)1 << p) / 32);
    // register ranges: up to about eight workgroups per CU over the launch, ranges of 64 words at least, the partial
    // counts within the budget
    auto part_bytes = [&](int rr) { return (size_t)rr * tsum * ((size_t)4 << n); };
    int RR = 1;
    while (RR < 64 && words / (2 * RR) >= SS_DMAX && base * 2 * RR <= 2048 && part_bytes(2 * RR) <= part_budget) RR *= 2;
    pl.RR = RR;
    const size_t per = words / RR;
    pl.D = (int)std::min<size_t>(per, SS_DMAX);
    pl.tiles = (int)(per / pl.D);
    pl.part_bytes = std::max<size_t>(part_bytes(RR), 4);
    pl.lds_bytes = (size_t)n * std::max(1, SS_WAVES / pl.nchunks + 1) * std::max(pl.D, 4) * 4;
    return pl;
}

void launch_subsets(const uint8_t* leaf_dev, int n, int K, int p, int k0, int Kc, const SubsetsPlan& pl, const int32_t* wg_dev,
                    const uint32_t* rng_dev, uint32_t* part_dev, uint32_t* hist_dev, hipStream_t st) {
    const unsigned nwg = (unsigned)(pl.wg.size() / 3);
    if (nwg) {
        const dim3 grid(nwg, (unsigned)pl.RR);
#define DD_SUBSETS_LAUNCH(HC) \
    launch_full_lds<subsets_kernel<HC>>(grid, dim3(SS_THREADS), pl.lds_bytes, st, leaf_dev, n, K, p, rng_dev, wg_dev, pl.nchunks, pl.D, pl.tiles, part_dev)
        switch (pl.HC) {
            case 1: DD_SUBSETS_LAUNCH(1); break;
            case 2: DD_SUBSETS_LAUNCH(2); break;
            case 4: DD_SUBSETS_LAUNCH(4); break;
            case 8: DD_SUBSETS_LAUNCH(8); break;
            case 16: DD_SUBSETS_LAUNCH(16); break;
            case 32: DD_SUBSETS_LAUNCH(32); break;
            default: DD_SUBSETS_LAUNCH(64); break;
        }
#undef DD_SUBSETS_LAUNCH
    }
    const size_t threads = (size_t)Kc << n;
    hipLaunchKernelGGL(subsets_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, part_dev, n, p, k0, Kc,
                       rng_dev, pl.RR, hist_dev);
}

}  // namespace dd
