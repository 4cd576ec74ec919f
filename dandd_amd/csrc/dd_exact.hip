// dd_exact.hip -- exact number of distinct (canonical) k-mers on the GPU: the KMC stand-in.
//
// Replaces  kmc -ci1 -cs2 -k<K> [-b] -fm <fasta> <db> <tmp>  +  kmc_tools complex (union)  +
// kmc_tools info | grep 'total k-mers'   (/root/reference/lib/sketch_classes.py:395,444-448,453-465):
// every k-mer occurrence of the token stream is materialised (8 or 16 bytes), radix-sorted
// (rocPRIM device radix sort over the 2k significant bits) and the distinct values are counted.
// This is the accuracy yardstick of the benchmark ("delta rel-err vs KMC --exact") and the
// engine's answer to `dandd tree --exact`; it is HBM-bound on the sort passes.
#include <string.h>

#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_exact_walk.h"

namespace dd {
namespace {

// Partition of the k-mer space for inputs whose k-mers do not fit the HBM budget at once: 4096 bins by a mix
// of the k-mer itself, so equal k-mers always share a bin and the distinct count is the sum over bins.
constexpr int kExactBinBits = 12;
DD_D uint32_t exact_bin(uint64_t lo, uint64_t hi) { return (uint32_t)(splitmix64(lo ^ (hi * 0x9E3779B97F4A7C15ull)) >> (64 - kExactBinBits)); }

// one thread per 64-token segment.
//   MODE 0: the k-mer ending at token t goes to out[base + t] (everything at once; unwritten slots keep a sentinel)
//   MODE 1: only counts k-mers per bin into hist[4096] (LDS histogram per workgroup, one flush)
//   MODE 2: k-mers whose bin is in [bin_lo, bin_hi) are appended densely (wave-aggregated atomic on counters[3])
//   TAG (modes 0 and 2; the union schedules of dd_exact_sched.hip): every k-mer carries the index of its genome
//   (blockIdx.y), 1: in the top byte of its most significant word (free while 2k, or 2k - 64, is at most 56),
//   2: as a byte of out_g next to the key.  Unwritten slots keep 0xFF there: a genome that sets no bit.
template <bool CANON, bool WIDE, int MODE, int TAG>
__global__ __launch_bounds__(256) void kmer_extract_kernel(const ExactGenome* __restrict__ tab, int k,
                                                          uint64_t* __restrict__ out_lo,
                                                          uint64_t* __restrict__ out_hi,
                                                          unsigned long long* __restrict__ counters,
                                                          unsigned long long* __restrict__ hist, uint32_t bin_lo,
                                                          uint32_t bin_hi, uint8_t* __restrict__ out_g) {
    __shared__ uint32_t lhist[MODE == 1 ? (1 << kExactBinBits) : 1];
    if (MODE == 1) {
        for (int i = threadIdx.x; i < (1 << kExactBinBits); i += blockDim.x) lhist[i] = 0;
        __syncthreads();
    }
    const ExactGenome g = tab[blockIdx.y];
    const unsigned long long seg = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const KeyMasks km = key_masks(k);
    unsigned valid = 0, allt = 0;
    // the sort, not this kernel, is the cost.  (MODE 2 keeps every lane in the token loop: the append is a wave-level operation)
    walk_segment<CANON, MODE == 2>(g.codes, g.bad, *g.ntok, seg, k, [&](unsigned long long sidx, int t, uint64_t ah, uint64_t al, bool have) {
        unsigned long long pos;
        if (MODE == 0) {
            pos = g.base + sidx * kSegTokens + (unsigned)t;
            ++valid;
            if (al == km.lo && ah == km.hi) allt = 1;
        } else {
            const uint32_t bin = exact_bin(al, WIDE ? ah : 0ull);
            if (MODE == 1) {
                atomicAdd(&lhist[bin], 1u);
                return;
            }
            const bool take = have && bin >= bin_lo && bin < bin_hi;
            pos = wave_append(take, &counters[3]);
            if (!take) return;
        }
        const uint64_t tag = (TAG == 1) ? (uint64_t)blockIdx.y << 56 : 0ull;
        out_lo[pos] = WIDE ? al : (al | tag);
        if (WIDE) out_hi[pos] = ah | tag;
        if (TAG == 2) out_g[pos] = (uint8_t)blockIdx.y;
    });
    if (MODE == 1) {
        __syncthreads();
        for (int i = threadIdx.x; i < (1 << kExactBinBits); i += blockDim.x)
            if (lhist[i]) atomicAdd(&hist[i], (unsigned long long)lhist[i]);
        return;
    }
    if (MODE == 2) return;
    // wave-level reduction of the two statistics, one atomic per wave
    for (int d = 32; d > 0; d >>= 1) {
        valid += __shfl_down(valid, d);
        allt |= __shfl_down(allt, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (valid) atomicAdd(&counters[0], (unsigned long long)valid);
        if (allt) atomicOr(&counters[1], 1ull);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void count_unique_kernel(const uint64_t* __restrict__ lo,
                                                          const uint64_t* __restrict__ hi, size_t n,
                                                          uint64_t mlo, uint64_t mhi,
                                                          unsigned long long* __restrict__ counters) {
    unsigned cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        bool fresh = (i == 0);
        if (!fresh) {
            fresh = ((lo[i] ^ lo[i - 1]) & mlo) != 0;
            if (WIDE) fresh |= ((hi[i] ^ hi[i - 1]) & mhi) != 0;
        }
        cnt += fresh;
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&counters[2], (unsigned long long)cnt);
}

}  // namespace

void launch_kmer_extract(const ExactGenome* tab_dev, int ng, size_t max_segments, int k, int canonical,
                         uint64_t* lo, uint64_t* hi, unsigned long long* counters, hipStream_t st, int mode,
                         unsigned long long* hist, uint32_t bin_lo, uint32_t bin_hi, int tag, uint8_t* g) {
    if (ng <= 0 || !max_segments) return;
    const dim3 grid((unsigned)((max_segments + 255) / 256), (unsigned)ng), block(256);
    // the (mode, tag) the kernel is built for: mode 1 writes no k-mer and takes no tag
    const auto mode_tag = [&](const auto& f) {
        using std::integral_constant;
        switch (mode == 1 ? 3 : (mode ? 4 : 0) + std::min(std::max(tag, 0), 2)) {
            case 0: return f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
            case 1: return f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
            case 2: return f(integral_constant<int, 0>{}, integral_constant<int, 2>{});
            case 3: return f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
            case 4: return f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
            case 5: return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
            default: return f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
        }
    };
    dispatch_bool(canonical != 0, [&](auto cn) {
        dispatch_bool(k > 32, [&](auto wd) {
            mode_tag([&](auto md, auto tg) {
                hipLaunchKernelGGL((kmer_extract_kernel<decltype(cn)::value, decltype(wd)::value, decltype(md)::value, decltype(tg)::value>), grid,
                                   block, 0, st, tab_dev, k, lo, hi, counters, hist, bin_lo, bin_hi, g);
            });
        });
    });
}

// ---- the one ordered sort of the exact path --------------------------------------------------------------------------
namespace {

template <class F>
hipError_t sort_keys(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, F* f, F* f_alt, size_t n, int k, void* temp,
                     size_t tb, hipStream_t st) {
    hipError_t e;
    if (k <= 32) {
        const unsigned bits = (unsigned)(2 * k);
        return f ? rocprim::radix_sort_pairs(temp, tb, lo, lo_alt, f, f_alt, n, 0, bits, st) : rocprim::radix_sort_keys(temp, tb, lo, lo_alt, n, 0, bits, st);
    }
    // stable LSD over the 128-bit key: low word first, then the high word's 2k - 64 bits.  A pair sort carries ONE value
    // array, so each pass runs once more for the follower, in front: the same keys give the same permutation (the sort is
    // stable and deterministic).
    const unsigned bits = (unsigned)(2 * k - 64);
    if (f && (e = rocprim::radix_sort_pairs(temp, tb, lo, lo_alt, f, f_alt, n, 0, 64, st)) != hipSuccess) return e;
    if ((e = rocprim::radix_sort_pairs(temp, tb, lo, lo_alt, hi, hi_alt, n, 0, 64, st)) != hipSuccess) return e;
    if (f && (e = rocprim::radix_sort_pairs(temp, tb, hi_alt, hi, f_alt, f, n, 0, bits, st)) != hipSuccess) return e;
    return rocprim::radix_sort_pairs(temp, tb, hi_alt, hi, lo_alt, lo, n, 0, bits, st);
}

}  // namespace

size_t exact_sort_keys_temp_bytes(size_t n, int k, size_t follow_bytes) {
    size_t a = 0, b = 0, c = 0;
    uint64_t* nul = nullptr;
    uint8_t* nul8 = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, a, nul, nul, n, 0, 64);
    if (follow_bytes == 1) (void)rocprim::radix_sort_pairs(nullptr, b, nul, nul, nul8, nul8, n, 0, 64);
    if (k > 32 || follow_bytes == 8) (void)rocprim::radix_sort_pairs(nullptr, c, nul, nul, nul, nul, n, 0, 64);
    return std::max(a, std::max(b, c)) + 256;
}

hipError_t launch_exact_sort_keys(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, void* follow, void* follow_alt,
                                  size_t follow_bytes, size_t n, int k, void* temp, size_t temp_bytes, hipStream_t st) {
    if (follow && follow_bytes == 8)
        return sort_keys(lo, hi, lo_alt, hi_alt, static_cast<uint64_t*>(follow), static_cast<uint64_t*>(follow_alt), n, k, temp, temp_bytes, st);
    return sort_keys(lo, hi, lo_alt, hi_alt, static_cast<uint8_t*>(follow), static_cast<uint8_t*>(follow_alt), n, k, temp, temp_bytes, st);
}

size_t exact_sort_temp_bytes(size_t n, int k) { return exact_sort_keys_temp_bytes(n, k, 0); }

// Sorts (lo[, hi]) using (lo_alt[, hi_alt]) as the other half of the double buffer and adds the
// number of distinct values (compared on their 2k significant bits) to counters[2].
hipError_t launch_exact_sort_count(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, size_t n,
                                   int k, void* temp, size_t temp_bytes, unsigned long long* counters,
                                   hipStream_t st) {
    if (!n) return hipSuccess;
    const hipError_t e = launch_exact_sort_keys(lo, hi, lo_alt, hi_alt, nullptr, nullptr, 0, n, k, temp, temp_bytes, st);
    if (e != hipSuccess) return e;
    const KeyMasks km = key_masks(k);
    const size_t blocks = std::min<size_t>((n + 255) / 256, 4096);
    dispatch_bool(k > 32, [&](auto wd) {
        constexpr bool W = decltype(wd)::value;
        hipLaunchKernelGGL(count_unique_kernel<W>, dim3((unsigned)blocks), dim3(256), 0, st, W ? lo : lo_alt, W ? hi : nullptr, n, km.lo, km.hi, counters);
    });
    return hipGetLastError();
}

}  // namespace dd
