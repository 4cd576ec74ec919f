// dd_exact_api.hip -- the exact entry points of the C ABI (include/dandd_hip.h) that count: dd_exact_count*, the exact union
// schedules (dd_exact_pairwise / _progressive / _leave_out / _subsets), the exact intersection schedules (dd_exact_spectrum /
// _core_progressive / _select) and the exact greedy walk (dd_exact_greedy).  A schedule entry is its argument rules, its
// table, one exact_schedule call and a shaper of one k's accumulator; call frame, upload, K0 and pass driver: dd_exact_host.h.
// Host-side orchestration only; the kernels are in dd_exact.hip, dd_exact_sched.hip and dd_exact_greedy.hip.
#include "dd_exact_host.h"

extern "C" {

// ---------------------------------------------------- exact count (its own rules: n = 0 is legal)
int dd_exact_count_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k,
                          uint64_t* distinct) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 0 || !distinct || (n && (!fasta_dev || !nbytes))) return fail(DD_EINVAL, "null argument");
    if (k < 1 || k > 64) return fail(DD_EINVAL, "k=%d outside 1..64", k);
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    *distinct = 0;
    if (!n) return DD_OK;
    DeviceGuard guard(c->device);
    int rc;
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    if (!in.slots) return DD_OK;
    unsigned long long total = 0;
    rc = exact_passes(
        c, in, n, k, ExactLayout{"exact count", 0, dd::exact_sort_temp_bytes, nullptr},
        [&](const ExactArrays& a, size_t count) -> int {
            DD_HIP(dd::launch_exact_sort_count(a.lo, a.hi, a.lo_alt, a.hi_alt, count, k, a.temp, a.temp_bytes, a.counters, c->stream));
            return DD_OK;
        },
        [&](const unsigned long long* h, bool single) {
            total += h[2];   // distinct = sum over passes
            if (!single) return;
            // the all-ones group holds the sentinels of unwritten slots and/or genuine T^k k-mers
            const bool sentinel_present = h[0] < (unsigned long long)in.slots, all_t = h[1] != 0;
            total = total - ((sentinel_present || all_t) ? 1 : 0) + (all_t ? 1 : 0);
        });
    if (rc) return rc;
    *distinct = total;
    return DD_OK;
}

int dd_exact_count(dd_ctx* c, const char* const* paths, int n, int k, uint64_t* distinct) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 0 || !distinct || (n && !paths)) return fail(DD_EINVAL, "null argument");
    return exact_upload_files(c, paths, n, [&](auto p, auto s) { return dd_exact_count_device(c, p, s, n, k, distinct); });
}

}  // extern "C"

// ------------------------------------------------------------------- exact union schedules
// dd_exact_sched.hip: one sort of the universe per k, a membership mask per distinct k-mer, one accumulator per schedule.
// (outside the C linkage: the driver is a template over the two forms of a schedule)
namespace {

using Acc = std::vector<unsigned long long>;   // one k's accumulator, exact_sched_acc_words() counts
// what a caller of exact_schedule does around the loop over k (dd_exact_greedy: its mask store); with an ExactSched only --
// a wide schedule that is given hooks is refused, not run without them
struct ScheduleHooks {
    std::function<int(const ExactInputs&, dd::ExactSched&)> begin;   // the inputs are packed and hold a token
    std::function<int(int kk, const Acc& acc)> after_k;              // k = kmin + kk is done and waited for
};
// ... and with the accumulators once every k is done: that of k = kmin + kk, of K, into the caller's array
using ScheduleShape = std::function<void(const Acc& acc, size_t kk, size_t K)>;

// the two forms of a schedule behind the sort: a 64-bit mask per distinct k-mer (dd_exact_sched.hip), a row of up to four
// words (dd_exact_wide.hip)
size_t sched_words(const dd::ExactSched& s) { return dd::exact_sched_acc_words(s); }
size_t sched_words(const dd::ExactWide& s) { return dd::exact_wide_acc_words(s); }
hipError_t sched_launch(const dd::ExactSorted& sorted, size_t count, int k, const dd::ExactSched& s, void* scratch, hipStream_t st) {
    return dd::launch_exact_sched(sorted, count, k, s, scratch, st);
}
hipError_t sched_launch(const dd::ExactSorted& sorted, size_t count, int k, const dd::ExactWide& s, void* scratch, hipStream_t st) {
    return dd::launch_exact_wide(sorted, count, k, s, scratch, st);
}
constexpr auto sched_scratch(const dd::ExactSched&) { return dd::exact_sched_scratch_bytes; }
constexpr auto sched_scratch(const dd::ExactWide&) { return dd::exact_wide_scratch_bytes; }

// The driver behind every schedule: K0 once, then for every k extract (with the genome's index) -> sort -> reduce +
// accumulate through exact_passes, on the context's device.  Nothing reaches `shape` before every k is done.
template <class Sched>
int exact_schedule(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, Sched s,
                   const std::vector<uint64_t>& table, const ScheduleShape& shape, const ScheduleHooks* hooks = nullptr) {
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    const size_t words = sched_words(s);
    std::vector<Acc> out((size_t)(kmax - kmin + 1), Acc(words, 0ull));
    const auto done = [&] {
        for (size_t kk = 0; shape && kk < out.size(); ++kk) shape(out[kk], kk, out.size());
        return DD_OK;
    };
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    c->st_blocks = 0;
    if (!in.slots) return done();   // (no input holds a token: every count is 0)
    if ((rc = c->hist.reserve(words * sizeof(unsigned long long)))) return rc;
    s.acc = static_cast<unsigned long long*>(c->hist.p);
    if (!table.empty()) {
        if ((rc = stage_table(c, c->ord, table.data(), table.size() * sizeof(uint64_t)))) return rc;
        s.table = static_cast<const uint64_t*>(c->ord.p);
    }
    if constexpr (std::is_same_v<Sched, dd::ExactSched>) {
        if (hooks && (rc = hooks->begin(in, s))) return rc;
    } else if (hooks) {
        return fail(DD_EINVAL, "exact schedule: hooks stand behind the one-word form only");   // (begin takes an ExactSched)
    }
    int most_passes = 0;
    for (int k = kmin; k <= kmax; ++k) {
        DD_HIP(hipMemsetAsync(s.acc, 0, words * sizeof(unsigned long long), st));
        rc = exact_sorted_passes(
            c, in, n, k, "exact schedule",
            [&](const dd::ExactSorted& sorted, size_t count, void* scratch) { return sched_launch(sorted, count, k, s, scratch, st); },
            sched_scratch(s));
        if (rc) return rc;
        DD_HIP(hipMemcpyAsync(out[(size_t)(k - kmin)].data(), s.acc, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        most_passes = std::max(most_passes, c->st_blocks);
        if (hooks && (rc = hooks->after_k(k - kmin, out[(size_t)(k - kmin)]))) return rc;
    }
    c->st_blocks = most_passes;   // (dd_last_sketch_stats: the passes of the k that took the most)
    return done();
}

// the schedules' argument rules (those of the HLL forms) and what they hand the accumulators
int progressive_table(const int32_t* orderings, int norder, int n, std::vector<uint64_t>& table) {
    if (norder < 1 || !orderings) return fail(DD_EINVAL, "bad argument");
    table.assign((size_t)norder * n, 0ull);
    for (int o = 0; o < norder; ++o) {
        uint64_t seen = 0;
        for (int j = 0; j < n; ++j) {
            const int32_t v = orderings[(size_t)o * n + j];
            if (v < 0 || v >= n) return fail(DD_EINVAL, "ordering entry %d outside 0..%d", v, n - 1);
            if ((seen >> v) & 1ull) return fail(DD_EINVAL, "ordering %d is not a permutation of 0..%d: %d appears twice", o, n - 1, v);
            seen |= 1ull << v;
            table[(size_t)o * n + j] = seen;
        }
    }
    return DD_OK;
}

int leave_out_table(const int32_t* group, int ngroups, int n, std::vector<uint64_t>& table) {
    if (!group) return fail(DD_EINVAL, "bad argument");
    if (check_groups(group, ngroups, n)) return DD_EINVAL;
    table.assign((size_t)64 + ngroups, 0ull);
    for (int i = 0; i < 64; ++i) table[i] = ~0ull;
    const uint64_t all = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    for (int i = 0; i < n; ++i) {
        if (group[i] < 0) continue;
        table[i] = (uint64_t)group[i];
        table[64 + group[i]] |= 1ull << i;
    }
    for (int g = 0; g < ngroups; ++g)
        if (table[64 + g] == all) return fail(DD_EINVAL, "group %d holds every leaf: the union of the rest is empty", g);
    return DD_OK;
}

// ... and the same rules and messages for rows of W = exact_wide_words(n) words (the wide entries, n <= 255)
int wide_progressive_table(const int32_t* orderings, int norder, int n, std::vector<uint64_t>& table) {
    if (norder < 1 || !orderings) return fail(DD_EINVAL, "bad argument");
    const size_t W = (size_t)dd::exact_wide_words(n);
    table.assign((size_t)norder * n * W, 0ull);
    for (int o = 0; o < norder; ++o) {
        uint64_t seen[4] = {0, 0, 0, 0};
        for (int j = 0; j < n; ++j) {
            const int32_t v = orderings[(size_t)o * n + j];
            if (v < 0 || v >= n) return fail(DD_EINVAL, "ordering entry %d outside 0..%d", v, n - 1);
            if ((seen[v >> 6] >> (v & 63)) & 1ull) return fail(DD_EINVAL, "ordering %d is not a permutation of 0..%d: %d appears twice", o, n - 1, v);
            seen[v >> 6] |= 1ull << (v & 63);
            for (size_t w = 0; w < W; ++w) table[((size_t)o * n + j) * W + w] = seen[w];
        }
    }
    return DD_OK;
}

int wide_leave_out_table(const int32_t* group, int ngroups, int n, std::vector<uint64_t>& table) {
    if (!group) return fail(DD_EINVAL, "bad argument");
    if (check_groups(group, ngroups, n)) return DD_EINVAL;
    const size_t W = (size_t)dd::exact_wide_words(n);
    table.assign((size_t)256 + (size_t)ngroups * W, 0ull);
    for (int i = 0; i < 256; ++i) table[i] = ~0ull;
    std::vector<int> members((size_t)ngroups, 0);
    for (int i = 0; i < n; ++i) {
        if (group[i] < 0) continue;
        table[i] = (uint64_t)group[i];
        table[(size_t)256 + (size_t)group[i] * W + (i >> 6)] |= 1ull << (i & 63);
        ++members[(size_t)group[i]];
    }
    for (int g = 0; g < ngroups; ++g)
        if (members[(size_t)g] == n) return fail(DD_EINVAL, "group %d holds every leaf: the union of the rest is empty", g);
    return DD_OK;
}

// accumulator counts -> the cards of the ABI
void pairwise_cards(const Acc& acc, int n, size_t kk, size_t K, uint64_t* card) {
    auto at = [n](int i, int j) { return (size_t)1 + (size_t)i * n - (size_t)i * (i - 1) / 2 + (size_t)(j - i); };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int a = std::min(i, j), b = std::max(i, j);
            const unsigned long long ci = acc[at(a, a)], cj = acc[at(b, b)];
            card[((size_t)i * n + j) * K + kk] = a == b ? ci : ci + cj - acc[at(a, b)];
        }
}

// progressive (forward): |union of the first j+1| = k-mers whose first genome stands at a position <= j;
// core-progressive (backward): |core of the first j+1| = k-mers whose last contained prefix stands at a position >= j
void running_sums(const Acc& acc, int n, int norder, bool forward, size_t kk, size_t K, uint64_t* out) {
    for (int o = 0; o < norder; ++o) {
        uint64_t run = 0;
        for (int i = 0; i < n; ++i) {
            const int j = forward ? i : n - 1 - i;
            run += acc[1 + (size_t)o * n + j];
            out[((size_t)o * n + j) * K + kk] = run;
        }
    }
}

// spectrum, select: the `rows` counts behind M as they are
void copy_rows(const Acc& acc, int rows, size_t kk, size_t K, uint64_t* out) {
    for (int j = 0; j < rows; ++j) out[(size_t)j * K + kk] = acc[1 + j];
}

int subsets_from_hist(const unsigned long long* hist, int n, uint64_t* card, size_t stride) {
    const size_t nsub = (size_t)1 << n;
    std::vector<uint64_t> sub(hist, hist + nsub);
    uint64_t total = 0;
    for (size_t s = 0; s < nsub; ++s) total += sub[s];
    for (int b = 0; b < n; ++b)   // subset-sum (zeta) transform: sub[T] = sum of hist[mask] over mask inside T
        for (size_t s = 0; s < nsub; ++s)
            if (s & ((size_t)1 << b)) sub[s] += sub[s ^ ((size_t)1 << b)];
    for (size_t s = 0; s < nsub; ++s) card[s * stride] = total - sub[(nsub - 1) ^ s];
    return DD_OK;
}

}  // namespace

extern "C" {

int dd_exact_pairwise_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, card)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedPairwise, n, 0, 0, nullptr, nullptr}, {},
                          [&](const Acc& a, size_t kk, size_t K) { pairwise_cards(a, n, kk, K, card); });
}

int dd_exact_progressive_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                const int32_t* orderings, int norder, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, card)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (progressive_table(orderings, norder, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedProgressive, n, norder, 0, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) { running_sums(a, n, norder, true, kk, K, card); });
}

int dd_exact_leave_out_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                              const int32_t* group, int ngroups, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, card)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (leave_out_table(group, ngroups, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedLeaveOut, n, 0, ngroups, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) {
                              for (int g = 0; g < ngroups; ++g) card[(size_t)g * K + kk] = a[0] - a[1 + g];
                              card[(size_t)ngroups * K + kk] = a[0];
                          });
}

int dd_exact_subsets_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 16, kmin, kmax, card)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSubsets, n, 0, 0, nullptr, nullptr}, {},
                          [&](const Acc& a, size_t kk, size_t K) { subsets_from_hist(a.data() + 1, n, card + kk, K); });
}

// ------------------------------------------------------- exact union schedules, 65 to 255 inputs
// dd_exact_wide.hip: the same sort, a row of up to four words per distinct k-mer.  The entries above keep their limit and
// their messages; these take their argument lists and output shapes, and any n in 1..255.
int dd_exact_wide_pairwise_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 255, kmin, kmax, card)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactWide{dd::kSchedPairwise, n, 0, 0, nullptr, nullptr}, {},
                          [&](const Acc& a, size_t kk, size_t K) { pairwise_cards(a, n, kk, K, card); });
}

int dd_exact_wide_progressive_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                     const int32_t* orderings, int norder, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 255, kmin, kmax, card)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (wide_progressive_table(orderings, norder, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactWide{dd::kSchedProgressive, n, norder, 0, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) { running_sums(a, n, norder, true, kk, K, card); });
}

int dd_exact_wide_leave_out_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                   const int32_t* group, int ngroups, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 255, kmin, kmax, card)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (wide_leave_out_table(group, ngroups, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactWide{dd::kSchedLeaveOut, n, 0, ngroups, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) {
                              for (int g = 0; g < ngroups; ++g) card[(size_t)g * K + kk] = a[0] - a[1 + g];
                              card[(size_t)ngroups * K + kk] = a[0];
                          });
}

int dd_exact_wide_pairwise(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* card) {
    return exact_path_form(c, paths, n, 255, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_wide_pairwise_device(c, p, s, n, kmin, kmax, card); });
}

int dd_exact_wide_progressive(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* orderings, int norder, uint64_t* card) {
    return exact_path_form(c, paths, n, 255, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_wide_progressive_device(c, p, s, n, kmin, kmax, orderings, norder, card); });
}

int dd_exact_wide_leave_out(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* group, int ngroups, uint64_t* card) {
    return exact_path_form(c, paths, n, 255, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_wide_leave_out_device(c, p, s, n, kmin, kmax, group, ngroups, card); });
}

// ---------------------------------------------------------------- exact intersection schedules
int dd_exact_spectrum_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* spec) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, spec)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSpectrum, n, 0, 0, nullptr, nullptr}, {},
                          [&](const Acc& a, size_t kk, size_t K) { copy_rows(a, n + 1, kk, K, spec); });
}

int dd_exact_core_progressive_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                     const int32_t* orderings, int norder, uint64_t* core) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, core)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (progressive_table(orderings, norder, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedCoreProgressive, n, norder, 0, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) { running_sums(a, n, norder, false, kk, K, core); });
}

int dd_exact_select_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                           const uint64_t* all, const uint64_t* none, int nq, uint64_t* count) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, count)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (select_table(all, none, nq, n, table)) return DD_EINVAL;
    return exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSelect, n, nq, 0, nullptr, nullptr}, table,
                          [&](const Acc& a, size_t kk, size_t K) { copy_rows(a, nq, kk, K, count); });
}

// ------------------------------------------------------------------------ exact greedy
// dd_exact_greedy.hip: the masks of every k kept in HBM (kSchedStream), one gains launch per step, the pick on the host.
namespace {

// c->masks: cursor, overflow word (256 B) | gains [64][64] u64 | the streams, k = kmin first
constexpr size_t kMaskHeadBytes = 256, kGainBytes = (size_t)dd::kGreedyMaxK * 64 * sizeof(unsigned long long);

// the walk: per step the gains of every input at every k, then dd_greedy's rule on |C|_k + gain
int greedy_walk(dd_ctx* c, const dd::GreedySegments& seg, int n, int kmin, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps,
                int32_t* order, uint64_t* card) {
    hipStream_t st = c->stream;
    const int K = seg.K;
    const unsigned long long total = seg.off[K];   // (0: no input holds a token, every union is empty)
    const size_t gbytes = (size_t)K * 64 * sizeof(unsigned long long);
    unsigned long long* gain_dev = total ? reinterpret_cast<unsigned long long*>(static_cast<char*>(c->masks.p) + kMaskHeadBytes) : nullptr;
    const uint64_t* store = total ? reinterpret_cast<const uint64_t*>(static_cast<char*>(c->masks.p) + kMaskHeadBytes + kGainBytes) : nullptr;
    std::vector<unsigned long long> gain((size_t)K * 64, 0ull), running((size_t)K, 0ull);
    std::vector<int32_t> left(cand + nfixed, cand + ncand), chosen_order((size_t)nsteps);   // left: in tie-break order throughout
    std::vector<uint64_t> cards((size_t)nsteps * K);
    std::vector<double> rows((size_t)ncand * K);
    uint64_t chosen = 0;
    for (int j = 0; j < nsteps; ++j) {
        if (total) {
            DD_HIP(hipMemsetAsync(gain_dev, 0, gbytes, st));
            {
                Span sp(c, DD_KERNEL_EXACT);
                dd::launch_exact_greedy_gains(store, seg, n, chosen, gain_dev, st);
            }
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(gain.data(), gain_dev, gbytes, hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));
        }
        const bool given = j < nfixed;
        const int32_t* from = given ? cand + j : left.data();
        const int nrows = given ? 1 : (int)left.size();
        for (int r = 0; r < nrows; ++r)
            for (int kk = 0; kk < K; ++kk) rows[(size_t)r * K + kk] = (double)(running[kk] + gain[(size_t)kk * 64 + from[r]]);
        const int pick = greedy_pick(rows.data(), nrows, K, kmin, mode);
        const int32_t g = from[pick];
        chosen_order[j] = g;
        for (int kk = 0; kk < K; ++kk) cards[(size_t)j * K + kk] = running[kk] += gain[(size_t)kk * 64 + g];
        chosen |= 1ull << g;
        if (!given) left.erase(left.begin() + pick);
    }
    memcpy(order, chosen_order.data(), sizeof(int32_t) * nsteps);   // (nothing is written before everything is known)
    memcpy(card, cards.data(), sizeof(uint64_t) * cards.size());
    return DD_OK;
}

}  // namespace

int dd_exact_greedy_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, int mode,
                           const int32_t* cand, int ncand, int nfixed, int nsteps, int32_t* order, uint64_t* card) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, kmin, kmax, card, !cand || !order)) return DD_EINVAL;
    if (check_greedy_walk(n, mode, cand, ncand, nfixed, nsteps)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    const int K = kmax - kmin + 1;
    const size_t budget = exact_budget("DD_EXACT_MASKS_MB");
    dd::GreedySegments seg{};   // off[kk]: where the stream of k = kmin + kk starts = the cursor when the k before it was done
    seg.K = K;
    size_t cap = 0;
    ScheduleHooks hooks;
    hooks.begin = [&](const ExactInputs& in, dd::ExactSched& s) -> int {
        cap = std::min(budget / sizeof(uint64_t), (size_t)K * in.slots);   // (a k holds no more distinct k-mers than the inputs have slots)
        if (c->masks.reserve(kMaskHeadBytes + kGainBytes + cap * sizeof(uint64_t)))
            return fail(DD_ENOMEM, "exact greedy: no device memory for a mask store of %zu masks (DD_EXACT_MASKS_MB sets its budget, %zu MiB now)",
                        cap, budget >> 20);
        char* mb = static_cast<char*>(c->masks.p);
        DD_HIP(hipMemsetAsync(mb, 0, kMaskHeadBytes, st));
        s.cursor = reinterpret_cast<unsigned long long*>(mb);
        s.overflow = s.cursor + 1;
        s.store = reinterpret_cast<uint64_t*>(mb + kMaskHeadBytes + kGainBytes);
        s.cap = cap;
        return DD_OK;
    };
    hooks.after_k = [&](int kk, const Acc& acc) -> int {
        unsigned long long h[2] = {0, 0};   // cursor, overflow
        DD_HIP(hipMemcpyAsync(h, c->masks.p, sizeof h, hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        if (h[1])
            return fail(DD_ENOMEM, "exact greedy: the mask streams of k = %d..%d need %llu masks, the store holds %zu (DD_EXACT_MASKS_MB sets its budget, %zu MiB now)",
                        kmin, kmin + kk, h[0], cap, budget >> 20);
        if (h[0] - seg.off[kk] != acc[0])
            return fail(DD_EHIP, "exact greedy: k=%d appended %llu masks to its stream, %llu distinct k-mers were counted", kmin + kk,
                        h[0] - seg.off[kk], acc[0]);
        seg.off[kk + 1] = h[0];
        return DD_OK;
    };
    int rc;
    const dd::ExactSched stream{dd::kSchedStream, n, 0, 0, nullptr, nullptr};
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, stream, {}, nullptr, &hooks))) return rc;
    return greedy_walk(c, seg, n, kmin, mode, cand, ncand, nfixed, nsteps, order, card);
}

// ------------------------------------------------------------------------ the path forms
int dd_exact_pairwise(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* card) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_pairwise_device(c, p, s, n, kmin, kmax, card); });
}

int dd_exact_progressive(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* orderings, int norder, uint64_t* card) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_progressive_device(c, p, s, n, kmin, kmax, orderings, norder, card); });
}

int dd_exact_leave_out(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* group, int ngroups, uint64_t* card) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_leave_out_device(c, p, s, n, kmin, kmax, group, ngroups, card); });
}

int dd_exact_subsets(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* card) {
    return exact_path_form(c, paths, n, 16, kmin, kmax, card,
                           [&](auto p, auto s) { return dd_exact_subsets_device(c, p, s, n, kmin, kmax, card); });
}

int dd_exact_spectrum(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* spec) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, spec,
                           [&](auto p, auto s) { return dd_exact_spectrum_device(c, p, s, n, kmin, kmax, spec); });
}

int dd_exact_core_progressive(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* orderings, int norder, uint64_t* core) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, core,
                           [&](auto p, auto s) { return dd_exact_core_progressive_device(c, p, s, n, kmin, kmax, orderings, norder, core); });
}

int dd_exact_select(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const uint64_t* all, const uint64_t* none, int nq, uint64_t* count) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, count,
                           [&](auto p, auto s) { return dd_exact_select_device(c, p, s, n, kmin, kmax, all, none, nq, count); });
}

int dd_exact_greedy(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, int mode, const int32_t* cand, int ncand, int nfixed,
                    int nsteps, int32_t* order, uint64_t* card) {
    return exact_path_form(c, paths, n, 64, kmin, kmax, card, [&](auto p, auto s) {
        return dd_exact_greedy_device(c, p, s, n, kmin, kmax, mode, cand, ncand, nfixed, nsteps, order, card);
    });
}

int dd_exact_subsets_from_hist(const uint64_t* hist, int n, uint64_t* card) {
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (!hist || !card) return fail(DD_EINVAL, "null argument");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
    return subsets_from_hist(reinterpret_cast<const unsigned long long*>(hist), n, card, 1);
}

}  // extern "C"
