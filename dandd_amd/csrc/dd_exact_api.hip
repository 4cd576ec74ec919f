// dd_exact_api.hip -- the exact entry points of the C ABI (include/dandd_hip.h): dd_exact_count*, the exact union
// schedules (dd_exact_pairwise / _progressive / _leave_out / _subsets), the exact intersection schedules
// (dd_exact_spectrum / _core_progressive / _select), the exact greedy walk (dd_exact_greedy), the selected k-mers
// themselves (dd_exact_select_kmers) and their positions (dd_exact_locate).  Host-side orchestration
// only; the kernels are in dd_exact.hip, dd_exact_sched.hip, dd_exact_greedy.hip and dd_exact_locate.hip.
#include <functional>
#include "dd_ctx.h"

using dd::FileBuf;
using dd::read_fasta_file;

namespace {

// K0 over the n inputs of an exact call (once per call, whatever the number of ks) and where each genome's k-mers go
struct ExactInputs {
    const dd::ExactGenome* etab_dev = nullptr;
    size_t slots = 0, max_segments = 0;   // slots = 0: no input has a token
    std::vector<dd::ExactGenome> etab;    // the host's copy of etab_dev (dd_exact_locate: where each stream and its ntok lie)
};

int exact_check_inputs(const uint8_t* const* fasta_dev, const size_t* nbytes, int n) {
    for (int g = 0; g < n; ++g) {
        if (nbytes[g] && !fasta_dev[g]) return fail(DD_EINVAL, "input %d: null buffer", g);
        if (reinterpret_cast<uintptr_t>(fasta_dev[g]) & 15)
            return fail(DD_EINVAL, "input %d: device buffer must be 16-byte aligned", g);
    }
    return DD_OK;
}

int exact_prepare(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, ExactInputs& in) {
    int rc;
    std::vector<unsigned long long> base(n);
    for (int g = 0; g < n; ++g) {
        base[g] = in.slots;
        const size_t segs = (nbytes[g] + dd::kSegTokens - 1) / dd::kSegTokens;
        in.slots += segs * dd::kSegTokens;
        in.max_segments = std::max(in.max_segments, segs);
    }
    if (!in.slots) return DD_OK;
    std::vector<dd::PackGenome> ptab;
    size_t max_chunks = 0;
    if ((rc = layout_tokens(c, fasta_dev, nbytes, n, ptab, max_chunks))) return rc;
    // K0's table and the extract's, one image: PackGenome[n] | ExactGenome[n], each 256-byte aligned
    const size_t pbytes = align_up(sizeof(dd::PackGenome) * n, 256), ebytes = align_up(sizeof(dd::ExactGenome) * n, 256);
    std::vector<char> image(pbytes + ebytes, 0);
    memcpy(image.data(), ptab.data(), sizeof(dd::PackGenome) * n);
    dd::ExactGenome* etab = reinterpret_cast<dd::ExactGenome*>(image.data() + pbytes);
    for (int g = 0; g < n; ++g) etab[g] = dd::ExactGenome{ptab[g].out.codes, ptab[g].out.bad, ptab[g].out.ntok, base[g]};
    in.etab.assign(etab, etab + n);
    if ((rc = stage_table(c, c->tables, image.data(), image.size()))) return rc;
    char* tdev = static_cast<char*>(c->tables.p);
    {
        Span sp(c, DD_KERNEL_PACK);
        dd::launch_pack_batch(reinterpret_cast<const dd::PackGenome*>(tdev), n, max_chunks, c->stream);
    }
    in.etab_dev = reinterpret_cast<const dd::ExactGenome*>(tdev + pbytes);
    return DD_OK;
}

size_t exact_budget() {
    size_t budget = (size_t)24 << 30;
    if (const char* e = getenv("DD_EXACT_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    return budget;
}

// the files of a path form, read and uploaded into the context's FASTA buffer
int exact_upload_files(dd_ctx* c, const char* const* paths, int n, std::vector<const uint8_t*>& ptrs, std::vector<size_t>& sizes) {
    std::vector<size_t> offs(n);
    std::vector<FileBuf> bufs(n);
    sizes.assign(n, 0);
    ptrs.assign(n, nullptr);
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        std::string err;
        if (!paths[i] || !read_fasta_file(paths[i], bufs[i], err, usable_cpus())) return fail(DD_EIO, "%s", err.c_str());
        sizes[i] = bufs[i].size();
        offs[i] = tot;
        tot += align_up(sizes[i] + 16, 256);
    }
    int rc;
    if ((rc = c->fasta.reserve(tot + 16))) return rc;
    for (int i = 0; i < n; ++i) {
        ptrs[i] = static_cast<const uint8_t*>(c->fasta.p) + offs[i];
        if (sizes[i])
            DD_HIP(hipMemcpyAsync(const_cast<uint8_t*>(ptrs[i]), bufs[i].data(), sizes[i], hipMemcpyHostToDevice, c->stream));
    }
    DD_HIP(hipStreamSynchronize(c->stream));  // host buffers are pageable; release them before the sort
    return DD_OK;
}

// ------------------------------------------------------------------------ the pass driver
// What a caller of exact_passes says about its part of the k-mer workspace.
struct ExactLayout {
    const char* what;                           // "exact count" / "exact schedule", for the messages
    int tag;                                    // launch_kmer_extract's tag mode; 2 adds the g | g_alt arrays (a byte per slot each)
    size_t (*temp_bytes)(size_t keys, int k);   // of the caller's sort
    size_t (*scratch_bytes)(size_t keys);       // what the caller wants behind the sort's temp (null: nothing)
};

// c->exact carved for `keys` k-mers:
// counters (256 B) | bin histogram (32 KiB) | lo | lo_alt [| hi | hi_alt] [| g | g_alt] | sort temp | scratch
struct ExactArrays {
    unsigned long long *counters, *hist;
    uint64_t *lo, *lo_alt, *hi, *hi_alt;   // hi: k > 32
    uint8_t *g, *g_alt;                    // tag mode 2
    void *temp, *scratch;
    size_t temp_bytes;
};

constexpr size_t kExactHistBytes = (size_t)dd::kExactBins * sizeof(unsigned long long);

int exact_carve(dd_ctx* c, const ExactLayout& L, int k, size_t keys, ExactArrays& a) {
    const bool wide = k > 32, sep = L.tag == 2;
    const size_t arrays = wide ? 4 : 2, stride = align_up(keys * sizeof(uint64_t), 256), gstride = sep ? align_up(keys, 256) : 0;
    a.temp_bytes = L.temp_bytes(keys, k);
    int rc = c->exact.reserve(256 + kExactHistBytes + arrays * stride + 2 * gstride + align_up(a.temp_bytes, 256) +
                              (L.scratch_bytes ? L.scratch_bytes(keys) : 0) + 256);
    if (rc) return rc;
    char* eb = static_cast<char*>(c->exact.p);
    a.counters = reinterpret_cast<unsigned long long*>(eb);
    a.hist = reinterpret_cast<unsigned long long*>(eb + 256);
    char* kb = eb + 256 + kExactHistBytes;
    a.lo = reinterpret_cast<uint64_t*>(kb);
    a.lo_alt = reinterpret_cast<uint64_t*>(kb + stride);
    a.hi = wide ? reinterpret_cast<uint64_t*>(kb + 2 * stride) : nullptr;
    a.hi_alt = wide ? reinterpret_cast<uint64_t*>(kb + 3 * stride) : nullptr;
    kb += arrays * stride;
    a.g = sep ? reinterpret_cast<uint8_t*>(kb) : nullptr;
    a.g_alt = sep ? reinterpret_cast<uint8_t*>(kb + gstride) : nullptr;
    kb += 2 * gstride;
    a.temp = kb;
    a.scratch = kb + align_up(a.temp_bytes, 256);
    return DD_OK;
}

// the counters of a pass, read back (dd_kernels.h, launch_kmer_extract); single: the pass held every slot of the inputs
using ExactCounted = std::function<void(const unsigned long long* h, bool single)>;

// The k-mers of the prepared inputs for one k, extracted into c->exact and handed to consume(arrays, count) -- which
// launches its sort and what follows -- everything at once when that fits exact_budget(), else in passes over disjoint
// parts of the k-mer space.  KMC unions arbitrarily many databases (lib/sketch_classes.py:453-465 of the reference); so
// must this.  The counters are zeroed before each pass, outside its timing span.  `counted` receives them after the
// pass; without it a single pass is not waited for.  c->st_blocks = the number of passes (dd_last_sketch_stats).
template <class Consume>
int exact_passes(dd_ctx* c, const ExactInputs& in, int n, int k, const ExactLayout& L, Consume consume, const ExactCounted& counted = nullptr) {
    hipStream_t st = c->stream;
    int rc;
    const bool wide = k > 32;
    const size_t slots = in.slots, per_slot = (wide ? 4 : 2) * sizeof(uint64_t) + (L.tag == 2 ? 2 : 0), budget = exact_budget();
    const bool single = per_slot * slots <= budget;
    size_t cap = single ? slots : std::max<size_t>(budget / per_slot, 4096);   // k-mers per pass
    ExactArrays a{};
    if ((rc = exact_carve(c, L, k, cap, a))) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    if (single) {
        DD_HIP(hipMemsetAsync(a.counters, 0, 256, st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            // unwritten slots read as the all-ones sentinel (T^k's run), with genome 0xFF, which sets no bit
            DD_HIP(hipMemsetAsync(a.lo, 0xFF, slots * sizeof(uint64_t), st));
            if (wide) DD_HIP(hipMemsetAsync(a.hi, 0xFF, slots * sizeof(uint64_t), st));
            if (a.g) DD_HIP(hipMemsetAsync(a.g, 0xFF, slots, st));
            dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, a.lo, a.hi, a.counters, st, 0, nullptr, 0, 0, L.tag, a.g);
            DD_HIP(hipGetLastError());
            if ((rc = consume(a, slots))) return rc;
        }
        if (counted) {
            DD_HIP(hipMemcpyAsync(h, a.counters, sizeof h, hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));
            counted(h, true);
        }
        c->st_blocks = 1;
        return DD_OK;
    }

    // ---- more k-mers than the budget holds: passes over disjoint parts of the k-mer space ------------
    // The k-mer space is cut into 4096 bins by a mix of the k-mer itself (equal k-mers share a bin), a
    // counting pass sizes the bins, consecutive bins are grouped into passes of at most `cap` k-mers, and every
    // pass extracts (densely), sorts and consumes only its own bins.
    DD_HIP(hipMemsetAsync(a.counters, 0, 256 + kExactHistBytes, st));
    {
        Span sp(c, DD_KERNEL_EXACT);
        dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, a.lo, a.hi, a.counters, st, 1, a.hist, 0, 0);
    }
    DD_HIP(hipGetLastError());
    std::vector<unsigned long long> bins(dd::kExactBins);
    DD_HIP(hipMemcpyAsync(bins.data(), a.hist, kExactHistBytes, hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    const unsigned long long biggest = *std::max_element(bins.begin(), bins.end());
    if (biggest > cap) {
        // one bin alone is over the budget (one k-mer repeated billions of times lands in one bin): the arrays
        // grow to hold it if the device has the room, otherwise this input cannot be counted here
        cap = (size_t)biggest;
        if (exact_carve(c, L, k, cap, a))
            return fail(DD_ENOMEM, "%s: one part of the k-mer space holds %llu k-mers, more than fits in HBM", L.what, biggest);
    }
    int npass = 0;
    for (uint32_t b0 = 0; b0 < (uint32_t)dd::kExactBins;) {
        unsigned long long in_pass = 0;
        uint32_t b1 = b0;
        while (b1 < (uint32_t)dd::kExactBins && in_pass + bins[b1] <= cap) in_pass += bins[b1++];
        if (in_pass) {
            DD_HIP(hipMemsetAsync(a.counters, 0, 256, st));
            {
                Span sp(c, DD_KERNEL_EXACT);
                dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, a.lo, a.hi, a.counters, st, 2, a.hist, b0, b1, L.tag, a.g);
                DD_HIP(hipGetLastError());
                // (every slot below in_pass is written: no sentinel, T^k is an ordinary value here)
                if ((rc = consume(a, (size_t)in_pass))) return rc;
            }
            DD_HIP(hipMemcpyAsync(h, a.counters, sizeof h, hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));
            if (h[3] != in_pass) return fail(DD_EHIP, "%s: pass over bins %u..%u appended %llu k-mers, %llu expected", L.what, b0, b1, h[3], in_pass);
            if (counted) counted(h, false);
            ++npass;
        }
        b0 = b1;
    }
    c->st_blocks = npass;
    return DD_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------- exact count
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
    DeviceGuard guard(c->device);
    std::vector<const uint8_t*> ptrs;
    std::vector<size_t> sizes;
    int rc;
    if ((rc = exact_upload_files(c, paths, n, ptrs, sizes))) return rc;
    return dd_exact_count_device(c, ptrs.data(), sizes.data(), n, k, distinct);
}

// ------------------------------------------------------------------- exact union schedules
// dd_exact_sched.hip: one sort of the universe per k, a membership mask per distinct k-mer, one accumulator per schedule.
namespace {

// what a caller of exact_schedule does around the loop over k (dd_exact_greedy: its mask store)
struct ScheduleHooks {
    std::function<int(const ExactInputs&, dd::ExactSched&)> begin;                             // the inputs are packed and hold a token
    std::function<int(int kk, const std::vector<unsigned long long>& acc)> after_k;            // k = kmin + kk is done and waited for
};

// The driver behind every schedule: K0 once, then for every k extract (with the genome's index) -> sort -> reduce +
// accumulate through exact_passes.  out[kk] receives the accumulator's exact_sched_acc_words() counts of k = kmin + kk.
int exact_schedule(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, dd::ExactSched s,
                   const std::vector<uint64_t>& table, std::vector<std::vector<unsigned long long>>& out,
                   const ScheduleHooks* hooks = nullptr) {
    hipStream_t st = c->stream;
    int rc;
    const size_t words = dd::exact_sched_acc_words(s);
    out.assign((size_t)(kmax - kmin + 1), std::vector<unsigned long long>(words, 0ull));
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    c->st_blocks = 0;
    if (!in.slots) return DD_OK;
    if ((rc = c->hist.reserve(words * sizeof(unsigned long long)))) return rc;
    s.acc = static_cast<unsigned long long*>(c->hist.p);
    if (!table.empty()) {
        if ((rc = stage_table(c, c->ord, table.data(), table.size() * sizeof(uint64_t)))) return rc;
        s.table = static_cast<const uint64_t*>(c->ord.p);
    }
    if (hooks && (rc = hooks->begin(in, s))) return rc;
    int most_passes = 0;
    for (int k = kmin; k <= kmax; ++k) {
        DD_HIP(hipMemsetAsync(s.acc, 0, words * sizeof(unsigned long long), st));
        rc = exact_passes(c, in, n, k, ExactLayout{"exact schedule", dd::exact_tag_mode(k), dd::exact_sched_temp_bytes, dd::exact_sched_scratch_bytes},
                          [&](const ExactArrays& a, size_t count) -> int {
                              dd::ExactSorted sorted{};
                              DD_HIP(dd::launch_exact_sort_tagged(a.lo, a.hi, a.lo_alt, a.hi_alt, a.g, a.g_alt, count, k, a.temp, a.temp_bytes, st, &sorted));
                              DD_HIP(dd::launch_exact_sched(sorted, count, k, s, a.scratch, st));
                              return DD_OK;
                          });
        if (rc) return rc;
        DD_HIP(hipMemcpyAsync(out[(size_t)(k - kmin)].data(), s.acc, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        most_passes = std::max(most_passes, c->st_blocks);
        if (hooks && (rc = hooks->after_k(k - kmin, out[(size_t)(k - kmin)]))) return rc;
    }
    c->st_blocks = most_passes;   // (dd_last_sketch_stats: the passes of the k that took the most)
    return DD_OK;
}

int exact_sched_args(dd_ctx* c, const void* inputs, int n, int nmax, int kmin, int kmax, const void* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || n > nmax)
        return nmax == 16 ? fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n)
                          : fail(DD_EINVAL, "n=%d outside 1..64: a membership mask has one bit per input", n);
    if (!inputs || !card) return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    return DD_OK;
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

// accumulator counts -> the cards of the ABI
void pairwise_cards(const std::vector<std::vector<unsigned long long>>& acc, int n, uint64_t* card) {
    const size_t K = acc.size();
    auto at = [n](int i, int j) { return (size_t)1 + (size_t)i * n - (size_t)i * (i - 1) / 2 + (size_t)(j - i); };
    for (size_t kk = 0; kk < K; ++kk)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const int a = std::min(i, j), b = std::max(i, j);
                const unsigned long long ci = acc[kk][at(a, a)], cj = acc[kk][at(b, b)];
                card[((size_t)i * n + j) * K + kk] = a == b ? ci : ci + cj - acc[kk][at(a, b)];
            }
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

// select's argument rules -> the (all, none) pairs its accumulator reads
int select_table(const uint64_t* all, const uint64_t* none, int nq, int n, std::vector<uint64_t>& table) {
    if (!all || !none) return fail(DD_EINVAL, "null argument");
    if (nq < 1) return fail(DD_EINVAL, "nq=%d: at least one query", nq);
    const uint64_t outside = n == 64 ? 0ull : ~((1ull << n) - 1ull);
    table.resize((size_t)2 * nq);
    for (int q = 0; q < nq; ++q) {
        if ((all[q] | none[q]) & outside) return fail(DD_EINVAL, "query %d: a bit outside 0..%d is set", q, n - 1);
        table[(size_t)2 * q] = all[q], table[(size_t)2 * q + 1] = none[q];
    }
    return DD_OK;
}

// a path form: the files read and uploaded, then the device form (which checks the schedule's own arguments)
extern "C++" template <class DeviceForm>
int exact_path_form(dd_ctx* c, const char* const* paths, int n, DeviceForm device_form) {
    DeviceGuard guard(c->device);
    for (int i = 0; i < n; ++i)
        if (!paths[i]) return fail(DD_EINVAL, "null argument");
    std::vector<const uint8_t*> ptrs;
    std::vector<size_t> sizes;
    int rc;
    if ((rc = exact_upload_files(c, paths, n, ptrs, sizes))) return rc;
    return device_form(ptrs.data(), sizes.data());
}

}  // namespace

int dd_exact_pairwise_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, card)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedPairwise, n, 0, 0, nullptr, nullptr}, {}, acc))) return rc;
    pairwise_cards(acc, n, card);
    return DD_OK;
}

int dd_exact_progressive_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                const int32_t* orderings, int norder, uint64_t* card) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, card)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (progressive_table(orderings, norder, n, table)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedProgressive, n, norder, 0, nullptr, nullptr}, table, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk)
        for (int o = 0; o < norder; ++o) {
            uint64_t run = 0;   // |union of the first j+1| = k-mers whose first genome stands at a position <= j
            for (int j = 0; j < n; ++j) {
                run += acc[kk][1 + (size_t)o * n + j];
                card[((size_t)o * n + j) * K + kk] = run;
            }
        }
    return DD_OK;
}

int dd_exact_leave_out_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                              const int32_t* group, int ngroups, uint64_t* card) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, card)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (leave_out_table(group, ngroups, n, table)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedLeaveOut, n, 0, ngroups, nullptr, nullptr}, table, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk) {
        for (int g = 0; g < ngroups; ++g) card[(size_t)g * K + kk] = acc[kk][0] - acc[kk][1 + g];
        card[(size_t)ngroups * K + kk] = acc[kk][0];
    }
    return DD_OK;
}

int dd_exact_subsets_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_sched_args(c, fasta_dev, n, 16, kmin, kmax, card)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSubsets, n, 0, 0, nullptr, nullptr}, {}, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk) subsets_from_hist(acc[kk].data() + 1, n, card + kk, K);
    return DD_OK;
}

// ---------------------------------------------------------------- exact intersection schedules
int dd_exact_spectrum_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, uint64_t* spec) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, spec)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSpectrum, n, 0, 0, nullptr, nullptr}, {}, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk)
        for (int j = 0; j <= n; ++j) spec[(size_t)j * K + kk] = acc[kk][1 + j];
    return DD_OK;
}

int dd_exact_core_progressive_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                                     const int32_t* orderings, int norder, uint64_t* core) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, core)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (progressive_table(orderings, norder, n, table)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedCoreProgressive, n, norder, 0, nullptr, nullptr}, table, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk)
        for (int o = 0; o < norder; ++o) {
            uint64_t run = 0;   // |core of the first j+1| = k-mers whose last contained prefix stands at a position >= j
            for (int j = n - 1; j >= 0; --j) {
                run += acc[kk][1 + (size_t)o * n + j];
                core[((size_t)o * n + j) * K + kk] = run;
            }
        }
    return DD_OK;
}

int dd_exact_select_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax,
                           const uint64_t* all, const uint64_t* none, int nq, uint64_t* count) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, count)) return DD_EINVAL;
    if (!nbytes) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    std::vector<uint64_t> table;
    if (select_table(all, none, nq, n, table)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedSelect, n, nq, 0, nullptr, nullptr}, table, acc))) return rc;
    const size_t K = acc.size();
    for (size_t kk = 0; kk < K; ++kk)
        for (int q = 0; q < nq; ++q) count[(size_t)q * K + kk] = acc[kk][1 + q];
    return DD_OK;
}

// ------------------------------------------------------------------------ exact greedy
// dd_exact_greedy.hip: the masks of every k kept in HBM (kSchedStream), one gains launch per step, the pick on the host.
namespace {

size_t exact_masks_budget() {
    size_t budget = (size_t)24 << 30;
    if (const char* e = getenv("DD_EXACT_MASKS_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    return budget;
}

// c->masks: cursor, overflow word (256 B) | gains [64][64] u64 | the streams, k = kmin first
constexpr size_t kMaskHeadBytes = 256, kGainBytes = (size_t)dd::kGreedyMaxK * 64 * sizeof(unsigned long long);

}  // namespace

int dd_exact_greedy_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, int mode,
                           const int32_t* cand, int ncand, int nfixed, int nsteps, int32_t* order, uint64_t* card) {
    if (exact_sched_args(c, fasta_dev, n, 64, kmin, kmax, card)) return DD_EINVAL;
    if (!nbytes || !cand || !order) return fail(DD_EINVAL, "null argument");
    if (check_greedy_walk(n, mode, cand, ncand, nfixed, nsteps)) return DD_EINVAL;
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    const int K = kmax - kmin + 1;
    const size_t budget = exact_masks_budget();
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
    hooks.after_k = [&](int kk, const std::vector<unsigned long long>& acc) -> int {
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
    std::vector<std::vector<unsigned long long>> acc;
    int rc;
    if ((rc = exact_schedule(c, fasta_dev, nbytes, n, kmin, kmax, dd::ExactSched{dd::kSchedStream, n, 0, 0, nullptr, nullptr}, {}, acc, &hooks))) return rc;

    // the walk: per step the gains of every input at every k, then dd_greedy's rule on |C|_k + gain
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

int dd_exact_greedy(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, int mode, const int32_t* cand, int ncand, int nfixed,
                    int nsteps, int32_t* order, uint64_t* card) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, card)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_greedy_device(c, p, s, n, kmin, kmax, mode, cand, ncand, nfixed, nsteps, order, card);
    });
}

// ------------------------------------------------------------------- the selected k-mers
// dd_exact_sched.hip, emit_kernel: the sort of the schedules for ONE k, then the k-mers whose mask matches a query leave for
// c->emit (cursor | lo | hi | mask) instead of being counted.  The chunks of the sort finish in any order and the passes
// each hold an arbitrary part of the k-mer space, so the records are sorted here, on the host, after the copy-back.
int dd_exact_select_kmers_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k, const uint64_t* all,
                                 const uint64_t* none, int nq, uint64_t* kmers, uint64_t* masks, size_t cap, uint64_t* found) {
    if (exact_sched_args(c, fasta_dev, n, 64, k, k, found)) return DD_EINVAL;
    if (!nbytes || (cap && (!kmers || !masks))) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    if (nq > dd::kEmitMaxQueries)
        return fail(DD_EINVAL, "nq=%d: at most %d queries in one call (what one launch holds); split them over calls", nq, dd::kEmitMaxQueries);
    std::vector<uint64_t> table;
    if (select_table(all, none, nq, n, table)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    *found = 0;
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    c->st_blocks = 0;
    if (!in.slots) return DD_OK;
    const size_t dcap = std::min(cap, in.slots), stride = align_up(dcap * sizeof(uint64_t), 256);   // (no more distinct k-mers than slots)
    if (c->emit.reserve(256 + 3 * stride))
        return fail(DD_ENOMEM, "exact select k-mers: no device memory for an output of %zu records (24 bytes each); ask with a smaller cap", dcap);
    char* eb = static_cast<char*>(c->emit.p);
    dd::ExactEmit e{n, nq, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<unsigned long long*>(eb), dcap};
    if (dcap) {
        e.lo = reinterpret_cast<uint64_t*>(eb + 256);
        e.hi = reinterpret_cast<uint64_t*>(eb + 256 + stride);
        e.mask = reinterpret_cast<uint64_t*>(eb + 256 + 2 * stride);
    }
    DD_HIP(hipMemsetAsync(eb, 0, 256, st));
    if ((rc = stage_table(c, c->ord, table.data(), table.size() * sizeof(uint64_t)))) return rc;
    e.table = static_cast<const uint64_t*>(c->ord.p);
    rc = exact_passes(c, in, n, k, ExactLayout{"exact select k-mers", dd::exact_tag_mode(k), dd::exact_sched_temp_bytes, dd::exact_sched_scratch_bytes},
                      [&](const ExactArrays& a, size_t count) -> int {
                          dd::ExactSorted sorted{};
                          DD_HIP(dd::launch_exact_sort_tagged(a.lo, a.hi, a.lo_alt, a.hi_alt, a.g, a.g_alt, count, k, a.temp, a.temp_bytes, st, &sorted));
                          DD_HIP(dd::launch_exact_emit(sorted, count, k, e, a.scratch, st));
                          return DD_OK;
                      });
    if (rc) return rc;
    unsigned long long total = 0;
    DD_HIP(hipMemcpyAsync(&total, e.cursor, sizeof total, hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    *found = total;
    if (!total || total > cap) return DD_OK;   // (more than the caller has room for: the count is the answer, nothing was kept whole)
    const bool wide = k > 32;
    const size_t m = (size_t)total;
    std::vector<uint64_t> lo(m), hi(wide ? m : 0), mk(m);
    DD_HIP(hipMemcpyAsync(lo.data(), e.lo, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (wide) DD_HIP(hipMemcpyAsync(hi.data(), e.hi, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipMemcpyAsync(mk.data(), e.mask, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    // ascending in the 2k-bit key: hi, then lo.  The keys are distinct, so the order is total and two calls agree byte for byte.
    struct Rec { uint64_t hi, lo, mask; };
    std::vector<Rec> rec(m);
    for (size_t i = 0; i < m; ++i) rec[i] = Rec{wide ? hi[i] : 0ull, lo[i], mk[i]};
    const auto before = [](const Rec& x, const Rec& y) { return x.hi != y.hi ? x.hi < y.hi : x.lo < y.lo; };
    // slices sorted side by side, then merged in pairs (every distinct k-mer of 16 x 5 Mbp is 20 M records)
    size_t parts = 1;
    while (parts * 2 <= (size_t)std::min(usable_cpus(), 16) && m / (parts * 2) >= ((size_t)1 << 16)) parts *= 2;
    const auto cut = [&](size_t i) { return rec.begin() + (ptrdiff_t)(m / parts * i + std::min(i, m % parts)); };
    const auto side_by_side = [](size_t jobs, const std::function<void(size_t)>& job) {
        std::vector<std::thread> th;
        for (size_t j = 1; j < jobs; ++j) th.emplace_back(job, j);
        job(0);
        for (std::thread& t : th) t.join();
    };
    side_by_side(parts, [&](size_t j) { std::sort(cut(j), cut(j + 1), before); });
    for (size_t w = 1; w < parts; w *= 2)
        side_by_side(parts / (2 * w), [&](size_t j) { std::inplace_merge(cut(2 * w * j), cut(2 * w * j + w), cut(2 * w * j + 2 * w), before); });
    for (size_t i = 0; i < m; ++i) kmers[2 * i] = rec[i].lo, kmers[2 * i + 1] = rec[i].hi, masks[i] = rec[i].mask;
    return DD_OK;
}

int dd_exact_select_kmers(dd_ctx* c, const char* const* paths, int n, int k, const uint64_t* all, const uint64_t* none, int nq,
                          uint64_t* kmers, uint64_t* masks, size_t cap, uint64_t* found) {
    if (exact_sched_args(c, paths, n, 64, k, k, found)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_select_kmers_device(c, p, s, n, k, all, none, nq, kmers, masks, cap, found);
    });
}

// ------------------------------------------------------------------- where the selected k-mers lie
// dd_exact_locate.hip: dd_exact_select_kmers' sort and emission with the jobs' distinct (all, none) pairs as queries, the
// records of all passes put in key order on the device (c->exact, free by then, is the sort's other half and temp), then
// one walk of every painted genome that looks each k-mer up in them.  Nothing but the bitmaps comes back.
int dd_exact_locate_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k, const uint64_t* all,
                           const uint64_t* none, const int32_t* genome, int njobs, const uint64_t* off, uint64_t* hits, uint64_t* found) {
    if (exact_sched_args(c, fasta_dev, n, 64, k, k, found)) return DD_EINVAL;
    if (!nbytes || !all || !none || !genome || !off) return fail(DD_EINVAL, "null argument");
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    if (njobs < 1 || njobs > dd::kEmitMaxQueries)
        return fail(DD_EINVAL, "njobs=%d outside 1..%d (what one launch holds); split the jobs over calls", njobs, dd::kEmitMaxQueries);
    const uint64_t outside = n == 64 ? 0ull : ~((1ull << n) - 1ull);
    for (int j = 0; j < njobs; ++j) {
        if (genome[j] < 0 || genome[j] >= n) return fail(DD_EINVAL, "job %d: genome %d outside 0..%d", j, genome[j], n - 1);
        if ((all[j] | none[j]) & outside) return fail(DD_EINVAL, "job %d: a bit outside 0..%d is set", j, n - 1);
    }
    if (off[njobs] < off[0]) return fail(DD_EINVAL, "off[] must ascend");
    const uint64_t words = off[njobs] - off[0];   // (each job's own share is checked once the inputs' token counts are known)
    if (words && !hits) return fail(DD_EINVAL, "null argument");
    // the queries of the emission: the jobs' distinct pairs
    std::vector<std::pair<uint64_t, uint64_t>> pairs((size_t)njobs);
    for (int j = 0; j < njobs; ++j) pairs[(size_t)j] = {all[j], none[j]};
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const int nq = (int)pairs.size();
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    *found = 0;
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    c->st_blocks = 0;
    // every genome's ntok, for the shape of the answer
    std::vector<unsigned long long> ntok((size_t)n, 0ull);
    if (in.slots) {
        for (int g = 0; g < n; ++g) DD_HIP(hipMemcpyAsync(&ntok[(size_t)g], in.etab[(size_t)g].ntok, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
    }
    size_t max_segments = 0;
    for (int j = 0; j < njobs; ++j) {
        const uint64_t want = (ntok[(size_t)genome[j]] + dd::kSegTokens - 1) / dd::kSegTokens;
        if (off[j + 1] - off[j] != want)
            return fail(DD_EINVAL, "job %d: off[%d] - off[%d] = %llu words, %llu expected (input %d holds %llu tokens, 64 to a word)", j, j + 1, j,
                        (unsigned long long)(off[j + 1] - off[j]), (unsigned long long)want, genome[j], ntok[(size_t)genome[j]]);
        max_segments = std::max(max_segments, (size_t)want);
    }
    if (!in.slots) return DD_OK;   // (no input holds a token)
    // the emission of dd_exact_select_kmers_device, with room for every distinct k-mer the inputs can hold
    const size_t dcap = in.slots, stride = align_up(dcap * sizeof(uint64_t), 256);
    if (c->emit.reserve(256 + 3 * stride))
        return fail(DD_ENOMEM, "exact locate: no device memory for the %zu bytes of the record area (24 bytes per k-mer slot of the inputs)", 256 + 3 * stride);
    char* eb = static_cast<char*>(c->emit.p);
    dd::ExactEmit e{n, nq, nullptr, reinterpret_cast<uint64_t*>(eb + 256), reinterpret_cast<uint64_t*>(eb + 256 + stride),
                    reinterpret_cast<uint64_t*>(eb + 256 + 2 * stride), reinterpret_cast<unsigned long long*>(eb), dcap};
    DD_HIP(hipMemsetAsync(eb, 0, 256, st));
    // one image for both tables: (all, none) [nq][2] | LocateUnit[] -- the jobs of a genome, kLocateJobs to a unit
    std::vector<int> order((size_t)njobs);
    for (int j = 0; j < njobs; ++j) order[(size_t)j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return genome[x] < genome[y]; });
    std::vector<dd::LocateUnit> units;
    for (int j : order) {
        const dd::ExactGenome& eg = in.etab[(size_t)genome[j]];
        if (!ntok[(size_t)genome[j]]) continue;   // (an empty bitmap)
        if (units.empty() || units.back().ntok != eg.ntok || units.back().nj == dd::kLocateJobs) {
            units.push_back(dd::LocateUnit{});
            units.back().codes = eg.codes, units.back().bad = eg.bad, units.back().ntok = eg.ntok;
        }
        dd::LocateUnit& u = units.back();
        u.all[u.nj] = all[j], u.none[u.nj] = none[j], u.out[u.nj] = off[j] - off[0];
        ++u.nj;
    }
    const size_t pbytes = align_up(sizeof(uint64_t) * 2 * (size_t)nq, 256);
    std::vector<char> image(pbytes + sizeof(dd::LocateUnit) * units.size(), 0);
    for (int q = 0; q < nq; ++q) {
        uint64_t* t = reinterpret_cast<uint64_t*>(image.data()) + 2 * (size_t)q;
        t[0] = pairs[(size_t)q].first, t[1] = pairs[(size_t)q].second;
    }
    memcpy(image.data() + pbytes, units.data(), sizeof(dd::LocateUnit) * units.size());
    if ((rc = stage_table(c, c->ord, image.data(), image.size()))) return rc;
    e.table = static_cast<const uint64_t*>(c->ord.p);
    const dd::LocateUnit* units_dev = reinterpret_cast<const dd::LocateUnit*>(static_cast<const char*>(c->ord.p) + pbytes);
    if ((rc = c->hits.reserve(words * sizeof(uint64_t)))) return rc;
    uint64_t* hits_dev = static_cast<uint64_t*>(c->hits.p);
    rc = exact_passes(c, in, n, k, ExactLayout{"exact locate", dd::exact_tag_mode(k), dd::exact_sched_temp_bytes, dd::exact_sched_scratch_bytes},
                      [&](const ExactArrays& a, size_t count) -> int {
                          dd::ExactSorted sorted{};
                          DD_HIP(dd::launch_exact_sort_tagged(a.lo, a.hi, a.lo_alt, a.hi_alt, a.g, a.g_alt, count, k, a.temp, a.temp_bytes, st, &sorted));
                          DD_HIP(dd::launch_exact_emit(sorted, count, k, e, a.scratch, st));
                          return DD_OK;
                      });
    if (rc) return rc;
    unsigned long long total = 0;
    DD_HIP(hipMemcpyAsync(&total, e.cursor, sizeof total, hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    if (total > dcap) return fail(DD_EHIP, "exact locate: %llu records emitted, the inputs have %zu k-mer slots", total, dcap);
    if (!total || !words) {
        if (words) DD_HIP(hipMemsetAsync(hits_dev, 0, words * sizeof(uint64_t), st));   // nothing matches: no search
    } else {
        // (a pass holds an arbitrary part of the k-mer space and its chunks finish in any order: one ordering, after the last)
        if (c->exact.reserve(dd::exact_locate_order_bytes((size_t)total, k)))
            return fail(DD_ENOMEM, "exact locate: no device memory for the %zu bytes that put %llu records in order",
                        dd::exact_locate_order_bytes((size_t)total, k), total);
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(dd::launch_exact_locate_order(e.lo, e.hi, e.mask, (size_t)total, k, c->exact.p, st, &set));
        dd::launch_exact_locate(units_dev, (int)units.size(), max_segments, k, c->canonical, set, hits_dev, st);
        DD_HIP(hipGetLastError());
    }
    std::vector<uint64_t> host((size_t)words);
    if (words) DD_HIP(hipMemcpyAsync(host.data(), hits_dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    if (words) memcpy(hits + off[0], host.data(), words * sizeof(uint64_t));   // (nothing is written before everything is known)
    *found = total;
    return DD_OK;
}

int dd_exact_locate(dd_ctx* c, const char* const* paths, int n, int k, const uint64_t* all, const uint64_t* none, const int32_t* genome,
                    int njobs, const uint64_t* off, uint64_t* hits, uint64_t* found) {
    if (exact_sched_args(c, paths, n, 64, k, k, found)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_locate_device(c, p, s, n, k, all, none, genome, njobs, off, hits, found);
    });
}

int dd_exact_spectrum(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* spec) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, spec)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) { return dd_exact_spectrum_device(c, p, s, n, kmin, kmax, spec); });
}

int dd_exact_core_progressive(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* orderings, int norder, uint64_t* core) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, core)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_core_progressive_device(c, p, s, n, kmin, kmax, orderings, norder, core);
    });
}

int dd_exact_select(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const uint64_t* all, const uint64_t* none, int nq, uint64_t* count) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, count)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_select_device(c, p, s, n, kmin, kmax, all, none, nq, count);
    });
}

int dd_exact_subsets_from_hist(const uint64_t* hist, int n, uint64_t* card) {
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (!hist || !card) return fail(DD_EINVAL, "null argument");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
    return subsets_from_hist(reinterpret_cast<const unsigned long long*>(hist), n, card, 1);
}

// host only: dd_io.h's record index of one file, in the caller's arrays
int dd_fasta_index(const char* path, uint64_t* seq_len, uint64_t* tok_start, size_t cap, uint64_t* nrec, char* names, size_t names_cap,
                   size_t* names_need, uint64_t* ntok) {
    if (!path || !nrec || !names_need || !ntok || (cap && (!seq_len || !tok_start)) || (names_cap && !names)) return fail(DD_EINVAL, "null argument");
    dd::FastaIndex ix;
    std::string err;
    if (!dd::fasta_index_file(path, ix, err, usable_cpus())) return fail(DD_EIO, "%s", err.c_str());
    size_t need = 0;
    for (const std::string& s : ix.names) need += s.size() + 1;
    *nrec = ix.seq_len.size(), *names_need = need, *ntok = ix.ntok;
    if (ix.seq_len.size() <= cap && !ix.seq_len.empty()) {
        memcpy(seq_len, ix.seq_len.data(), sizeof(uint64_t) * ix.seq_len.size());
        memcpy(tok_start, ix.tok_start.data(), sizeof(uint64_t) * ix.tok_start.size());
    }
    if (need <= names_cap)
        for (const std::string& s : ix.names) memcpy(names, s.c_str(), s.size() + 1), names += s.size() + 1;
    return DD_OK;
}

int dd_exact_pairwise(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, card)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) { return dd_exact_pairwise_device(c, p, s, n, kmin, kmax, card); });
}

int dd_exact_progressive(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* orderings, int norder, uint64_t* card) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, card)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_progressive_device(c, p, s, n, kmin, kmax, orderings, norder, card);
    });
}

int dd_exact_leave_out(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, const int32_t* group, int ngroups, uint64_t* card) {
    if (exact_sched_args(c, paths, n, 64, kmin, kmax, card)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) {
        return dd_exact_leave_out_device(c, p, s, n, kmin, kmax, group, ngroups, card);
    });
}

int dd_exact_subsets(dd_ctx* c, const char* const* paths, int n, int kmin, int kmax, uint64_t* card) {
    if (exact_sched_args(c, paths, n, 16, kmin, kmax, card)) return DD_EINVAL;
    return exact_path_form(c, paths, n, [&](const uint8_t* const* p, const size_t* s) { return dd_exact_subsets_device(c, p, s, n, kmin, kmax, card); });
}

}  // extern "C"
