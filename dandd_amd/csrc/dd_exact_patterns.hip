// dd_exact_patterns.hip -- the membership-pattern table behind the patterns accumulator of dd_exact_sched.hip.
//
// A pass of the pass driver leaves (mask, count) pairs in HBM, one per slot of a workgroup's LDS table at each flush, in the
// order the flushes reserved their places.  Here they become the table: radix-sorted by mask, equal masks reduced to one row
// with the sum of their counts (u64), the rows merged with the running table of the passes before -- both are in mask order,
// so that is one merge and one more reduce -- and, behind the last pass, the table put in answer order: a stable sort on the
// inverted count over the mask-ordered rows gives count descending with ties by mask ascending.  Sums of integers in any
// order: two calls give the same bytes.  All of it is rocPRIM on the caller's stream; the one kernel here inverts the counts.
#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>

#include <algorithm>

#include "dd_common.h"
#include "dd_kernels.h"

namespace dd {
namespace {

using u64 = uint64_t;
using ull = unsigned long long;
constexpr size_t kHeadBytes = 256;

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

size_t sort_temp(size_t rows) {
    size_t b = 0;
    u64* nk = nullptr;
    ull* nv = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, nk, nk, nv, nv, rows, 0, 64);
    return b;
}
size_t reduce_temp(size_t rows) {
    size_t b = 0;
    u64* nk = nullptr;
    ull* nv = nullptr;
    (void)rocprim::reduce_by_key(nullptr, b, nk, nv, rows, nk, nv, nv, rocprim::plus<ull>(), rocprim::equal_to<u64>());
    return b;
}
size_t merge_temp(size_t rows_a, size_t rows_b) {
    size_t b = 0;
    u64* nk = nullptr;
    ull* nv = nullptr;
    (void)rocprim::merge(nullptr, b, nk, nk, nk, nv, nv, nv, rows_a, rows_b, rocprim::less<u64>());
    return b;
}

__global__ __launch_bounds__(256) void invert_kernel(const ull* __restrict__ in, ull* __restrict__ out, size_t rows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) out[i] = ~in[i];
}

}  // namespace

size_t exact_patterns_stride(size_t rows) { return up256(rows * sizeof(u64)); }

// the schedule's scratch | head | masks | counts
size_t exact_patterns_scratch_bytes(size_t keys) {
    return up256(exact_sched_scratch_bytes(keys)) + kHeadBytes + 2 * exact_patterns_stride(keys);
}

size_t exact_patterns_temp_bytes(size_t keys, int k) {
    return std::max(exact_sched_temp_bytes(keys, k), std::max(sort_temp(keys), reduce_temp(keys)));
}

PatternPairs exact_patterns_pairs(void* scratch, size_t keys) {
    char* b = static_cast<char*>(scratch) + up256(exact_sched_scratch_bytes(keys));
    return PatternPairs{reinterpret_cast<ull*>(b), reinterpret_cast<u64*>(b + kHeadBytes),
                        reinterpret_cast<ull*>(b + kHeadBytes + exact_patterns_stride(keys)), keys, scratch};
}

hipError_t launch_patterns_reduce(const PatternPairs& p, size_t npairs, int n, u64* alt_mask, ull* alt_count, void* temp, size_t temp_bytes,
                                  hipStream_t st) {
    if (!npairs) return hipMemsetAsync(p.head + 4, 0, sizeof(ull), st);
    if (npairs > p.cap) return hipErrorInvalidValue;
    size_t tb = temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(temp, tb, p.mask, alt_mask, p.count, alt_count, npairs, 0, n, st);   // (a mask has n bits)
    if (e != hipSuccess) return e;
    tb = temp_bytes;
    return rocprim::reduce_by_key(temp, tb, alt_mask, alt_count, npairs, p.mask, p.count, p.head + 4, rocprim::plus<ull>(),
                                  rocprim::equal_to<u64>(), st);
}

// dst: masks | counts | merged masks | merged counts | row count (256 B) | temp
size_t exact_patterns_merge_bytes(size_t rows) {
    return 4 * exact_patterns_stride(rows) + kHeadBytes + up256(std::max(merge_temp(rows, rows), reduce_temp(rows)));
}

hipError_t launch_patterns_merge(const u64* mask_a, const ull* count_a, size_t rows_a, const u64* mask_b, const ull* count_b, size_t rows_b,
                                 void* dst, ull** rows_out, hipStream_t st) {
    const size_t rows = rows_a + rows_b, stride = exact_patterns_stride(rows);
    char* b = static_cast<char*>(dst);
    u64* out_mask = reinterpret_cast<u64*>(b);
    ull* out_count = reinterpret_cast<ull*>(b + stride);
    u64* all_mask = reinterpret_cast<u64*>(b + 2 * stride);
    ull* all_count = reinterpret_cast<ull*>(b + 3 * stride);
    *rows_out = reinterpret_cast<ull*>(b + 4 * stride);
    void* temp = b + 4 * stride + kHeadBytes;
    if (!rows) return hipMemsetAsync(*rows_out, 0, sizeof(ull), st);
    size_t tb = merge_temp(rows_a, rows_b);
    if (!rows_a || !rows_b) {   // nothing to merge with: the rows that are there, each mask once already
        const u64* m = rows_a ? mask_a : mask_b;
        const ull* c = rows_a ? count_a : count_b;
        const ull n = rows;
        hipError_t e = hipMemcpyAsync(out_mask, m, rows * sizeof(u64), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_count, c, rows * sizeof(ull), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(*rows_out, &n, sizeof n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // (n is a local)
        return e;
    }
    hipError_t e = rocprim::merge(temp, tb, mask_a, mask_b, all_mask, count_a, count_b, all_count, rows_a, rows_b, rocprim::less<u64>(), st);
    if (e != hipSuccess) return e;
    tb = reduce_temp(rows);
    return rocprim::reduce_by_key(temp, tb, all_mask, all_count, rows, out_mask, out_count, *rows_out, rocprim::plus<ull>(),
                                  rocprim::equal_to<u64>(), st);
}

// work: masks out | inverted counts out | inverted counts in | temp
size_t exact_patterns_order_bytes(size_t rows) { return 3 * exact_patterns_stride(rows) + up256(sort_temp(rows)); }

hipError_t launch_patterns_order(const u64* mask, const ull* count, size_t rows, void* work, hipStream_t st) {
    if (!rows) return hipSuccess;
    const size_t stride = exact_patterns_stride(rows);
    char* b = static_cast<char*>(work);
    u64* out_mask = reinterpret_cast<u64*>(b);
    ull* out_inv = reinterpret_cast<ull*>(b + stride);
    ull* inv = reinterpret_cast<ull*>(b + 2 * stride);
    hipLaunchKernelGGL(invert_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, count, inv, rows);
    size_t tb = sort_temp(rows);
    // (keys: the inverted counts, values: the masks; the radix sort is stable, the rows come in mask order)
    return rocprim::radix_sort_pairs(b + 3 * stride, tb, inv, out_inv, const_cast<u64*>(mask), out_mask, rows, 0, 64, st);
}

}  // namespace dd
