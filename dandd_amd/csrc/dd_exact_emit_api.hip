// dd_exact_emit_api.hip -- the exact entry points of the C ABI (include/dandd_hip.h) that hand k-mers out instead of counting
// them.  Seven look k-mers up in the ordered records of one emission: the selected k-mers themselves (dd_exact_select_kmers),
// where they lie in each genome (dd_exact_locate), what samples that are no inputs hold of them (dd_exact_screen), where
// along themselves (dd_exact_paint), which genome each of their records belongs to (dd_exact_reads), how many times they
// hold each (dd_exact_depth) and where along each genome, and how deep (dd_exact_cover).  Each is its own
// argument rules, the ordered-record step of dd_exact_host.h (exact_records, then ExactRecords::order inside the entry's
// timing span) and the kernels that read the ordered set; screen, paint, reads, depth and cover also share the frame below: K0
// over the universe and the samples, a sort that sees the universe only.
// dd_exact_patterns hands out no k-mer but is ragged like the others -- one k per call, a cap and a count -- and
// dd_fasta_index is the record index of a file that turns places into names.
// Host-side orchestration only; the kernels are in dd_exact_sched.hip (emit_kernel, AccPatterns), dd_exact_locate.hip,
// dd_exact_screen.hip, dd_exact_paint.hip, dd_exact_reads.hip, dd_exact_depth.hip, dd_exact_cover.hip and dd_exact_patterns.hip.
#include "dd_exact_host.h"

extern "C" {

// ------------------------------------------------------------------- the selected k-mers
// The sort of the schedules for ONE k, then the k-mers whose mask matches a query leave for c->emit instead of being counted.
// Chunks finish in any order and a pass holds an arbitrary part of the k-mer space, so the records are put in order afterwards,
// on the device: ascending in the 2k-bit key, hi then lo.  The keys are distinct: the order is total, two calls agree byte for byte.
int dd_exact_select_kmers_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k, const uint64_t* all,
                                 const uint64_t* none, int nq, uint64_t* kmers, uint64_t* masks, size_t cap, uint64_t* found) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, k, k, found, cap && (!kmers || !masks))) return DD_EINVAL;
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
    ExactRecords rec;   // (no more distinct k-mers than slots)
    if ((rc = exact_records(c, in, n, k, "exact select k-mers", nullptr, nq, table.data(), table.size() * sizeof(uint64_t), std::min(cap, in.slots), rec)))
        return rc;
    *found = rec.found;
    if (!rec.kept) return DD_OK;   // (none, or more than the caller has room for: the count is the answer)
    dd::LocateSet set{};
    {
        Span sp(c, DD_KERNEL_EXACT);
        DD_HIP(rec.order(c, k, &set));
    }
    const bool wide = k > 32;
    const size_t m = (size_t)rec.found;
    std::vector<uint64_t> lo(m), hi(wide ? m : 0), mk(m);
    DD_HIP(hipMemcpyAsync(lo.data(), set.lo, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (wide) DD_HIP(hipMemcpyAsync(hi.data(), set.hi, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipMemcpyAsync(mk.data(), set.mask, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < m; ++i) kmers[2 * i] = lo[i], kmers[2 * i + 1] = wide ? hi[i] : 0ull, masks[i] = mk[i];
    return DD_OK;
}

int dd_exact_select_kmers(dd_ctx* c, const char* const* paths, int n, int k, const uint64_t* all, const uint64_t* none, int nq,
                          uint64_t* kmers, uint64_t* masks, size_t cap, uint64_t* found) {
    return exact_path_form(c, paths, n, 64, k, k, found, [&](auto p, auto s) {
        return dd_exact_select_kmers_device(c, p, s, n, k, all, none, nq, kmers, masks, cap, found);
    });
}

// ------------------------------------------------------------------- where the selected k-mers lie
// dd_exact_locate.hip: the emission with the jobs' distinct (all, none) pairs as queries and room for every distinct k-mer
// the inputs can hold, the records put in key order, then one walk of every painted genome that looks each k-mer up in
// them.  Nothing but the bitmaps comes back.
namespace {

// every genome's ntok, for the shape of the answer: each job's share of off[] checked against it
int locate_shape(dd_ctx* c, const ExactInputs& in, int n, const int32_t* genome, int njobs, const uint64_t* off,
                 std::vector<unsigned long long>& ntok, size_t& max_segments) {
    int rc;
    if ((rc = exact_read_ntok(c, in, 0, n, ntok))) return rc;
    max_segments = 0;
    for (int j = 0; j < njobs; ++j) {
        const uint64_t want = (ntok[(size_t)genome[j]] + dd::kSegTokens - 1) / dd::kSegTokens;
        if (off[j + 1] - off[j] != want)
            return fail(DD_EINVAL, "job %d: off[%d] - off[%d] = %llu words, %llu expected (input %d holds %llu tokens, 64 to a word)", j, j + 1, j,
                        (unsigned long long)(off[j + 1] - off[j]), (unsigned long long)want, genome[j], ntok[(size_t)genome[j]]);
        max_segments = std::max(max_segments, (size_t)want);
    }
    return DD_OK;
}

// the jobs of a genome, kLocateJobs to a unit
void locate_units(const ExactInputs& in, const std::vector<unsigned long long>& ntok, const uint64_t* all, const uint64_t* none,
                  const int32_t* genome, int njobs, const uint64_t* off, std::vector<dd::LocateUnit>& units) {
    std::vector<int> order((size_t)njobs);
    for (int j = 0; j < njobs; ++j) order[(size_t)j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return genome[x] < genome[y]; });
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
}

}  // namespace

int dd_exact_locate_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k, const uint64_t* all,
                           const uint64_t* none, const int32_t* genome, int njobs, const uint64_t* off, uint64_t* hits, uint64_t* found) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, k, k, found, !all || !none || !genome || !off)) return DD_EINVAL;
    if (njobs < 1 || njobs > dd::kEmitMaxQueries)
        return fail(DD_EINVAL, "njobs=%d outside 1..%d (what one launch holds); split the jobs over calls", njobs, dd::kEmitMaxQueries);
    for (int j = 0; j < njobs; ++j) {
        if (genome[j] < 0 || genome[j] >= n) return fail(DD_EINVAL, "job %d: genome %d outside 0..%d", j, genome[j], n - 1);
        if (exact_check_bits("job", j, all[j], none[j], n)) return DD_EINVAL;
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
    std::vector<unsigned long long> ntok;
    size_t max_segments = 0;
    if ((rc = locate_shape(c, in, n, genome, njobs, off, ntok, max_segments))) return rc;
    if (!in.slots) return DD_OK;   // (no input holds a token)
    // one image for both tables: (all, none) [nq][2] | LocateUnit[]
    std::vector<dd::LocateUnit> units;
    locate_units(in, ntok, all, none, genome, njobs, off, units);
    const size_t pbytes = align_up(sizeof(uint64_t) * 2 * (size_t)nq, 256);
    std::vector<char> image(pbytes + sizeof(dd::LocateUnit) * units.size(), 0);
    for (int q = 0; q < nq; ++q) {
        uint64_t* t = reinterpret_cast<uint64_t*>(image.data()) + 2 * (size_t)q;
        t[0] = pairs[(size_t)q].first, t[1] = pairs[(size_t)q].second;
    }
    memcpy(image.data() + pbytes, units.data(), sizeof(dd::LocateUnit) * units.size());
    if ((rc = c->hits.reserve(words * sizeof(uint64_t)))) return rc;
    uint64_t* hits_dev = static_cast<uint64_t*>(c->hits.p);
    ExactRecords rec;
    if ((rc = exact_records(c, in, n, k, "exact locate", &kSlotsOfInputs, nq, image.data(), image.size(), in.slots, rec))) return rc;
    if (!rec.kept || !words) {
        if (words) DD_HIP(hipMemsetAsync(hits_dev, 0, words * sizeof(uint64_t), st));   // nothing matches: no search
    } else {
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(rec.order(c, k, &set));
        const dd::LocateUnit* units_dev = reinterpret_cast<const dd::LocateUnit*>(static_cast<const char*>(c->ord.p) + pbytes);
        dd::launch_exact_locate(units_dev, (int)units.size(), max_segments, k, c->canonical, set, hits_dev, st);
        DD_HIP(hipGetLastError());
    }
    std::vector<uint64_t> host((size_t)words);
    if (words) DD_HIP(hipMemcpyAsync(host.data(), hits_dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    if (words) memcpy(hits + off[0], host.data(), words * sizeof(uint64_t));   // (nothing is written before everything is known)
    *found = rec.found;
    return DD_OK;
}

int dd_exact_locate(dd_ctx* c, const char* const* paths, int n, int k, const uint64_t* all, const uint64_t* none, const int32_t* genome,
                    int njobs, const uint64_t* off, uint64_t* hits, uint64_t* found) {
    return exact_path_form(c, paths, n, 64, k, k, found, [&](auto p, auto s) {
        return dd_exact_locate_device(c, p, s, n, k, all, none, genome, njobs, off, hits, found);
    });
}

// ------------------------------------------------------------------- the universe and the samples: what screen, paint, reads and depth share
// K0 runs over the universe's n inputs AND the ns samples behind them, once.  The sort and the emission see the universe
// alone -- the samples stay out of the sort and out of the slot count that sizes the record area -- with the single query
// (0, 0); the entry's own table rides behind that query in the image the emission stages.
namespace {

// the argument rules of both, in front of the entry's own ...
int universe_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const void* found) {
    if (exact_args(c, inputs, n, 64, k, k, found)) return DD_EINVAL;
    if (ns < 1 || ns > 1024) return fail(DD_EINVAL, "ns=%d outside 1..1024 samples in one call; split them over calls", ns);
    return DD_OK;
}

// ... with the (all, none) queries of a tally over the records (screen, depth): 0..kScreenMaxQueries of them, their bits
// inside n; out_null: one of the entry's own outputs is missing
int universe_query_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* all, const uint64_t* none, int nq, bool out_null,
                        const void* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (nq < 0 || nq > dd::kScreenMaxQueries)
        return fail(DD_EINVAL, "nq=%d outside 0..%d (what one launch holds); split the queries over calls", nq, dd::kScreenMaxQueries);
    if (out_null || (nq && (!all || !none))) return fail(DD_EINVAL, "null argument");
    for (int q = 0; q < nq; ++q)
        if (exact_check_bits("query", q, all[q], none[q], n)) return DD_EINVAL;
    return DD_OK;
}

// ... and, in a device form, behind them
int universe_buffers(const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns) {
    return nbytes ? exact_check_inputs(fasta_dev, nbytes, n + ns) : fail(DD_EINVAL, "null argument");
}

// K0 over everything; then in.slots and in.max_segments are the universe's alone (in.slots = 0: it holds no token, nothing is
// sorted), while in.etab still lists the samples behind the universe
int universe_prepare(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, ExactInputs& in) {
    int rc;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n + ns, in))) return rc;
    c->st_blocks = 0;
    in.slots = 0, in.max_segments = 0;
    for (int g = 0; g < n; ++g) {
        const size_t segs = (nbytes[g] + dd::kSegTokens - 1) / dd::kSegTokens;
        in.slots += segs * dd::kSegTokens, in.max_segments = std::max(in.max_segments, segs);
    }
    return DD_OK;
}

// one image for both tables: the emission's single query (0, 0) | the entry's own table, kOwnTable bytes into the image on the
// host and into c->ord once it is staged
constexpr size_t kOwnTable = 256;
void* own_table(void* image) { return static_cast<char*>(image) + kOwnTable; }

// a path form behind the entry's argument rules: the universe's files and the samples read and uploaded as one list
int universe_path_form(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, const ExactDeviceForm& device_form) {
    if (!samples) return fail(DD_EINVAL, "null argument");
    std::vector<const char*> files((size_t)(n + ns));
    for (int i = 0; i < n + ns; ++i)
        if (!(files[(size_t)i] = i < n ? paths[i] : samples[i - n])) return fail(DD_EINVAL, "null argument");
    return exact_upload_files(c, files.data(), n + ns, device_form);
}

}  // namespace

// ------------------------------------------------------------------- samples screened against the universe
// dd_exact_screen.hip: the records of the universe put in key order, one walk of every sample that marks the records it
// holds, one tally of the marks.  The ordered set may lie in the exact workspace: no sort runs there before the tally has
// finished.
namespace {

int screen_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* all, const uint64_t* none, int nq,
                const uint64_t* shared, const uint64_t* match, const uint64_t* found) {
    return universe_query_args(c, inputs, n, ns, k, all, none, nq, !shared || (nq && !match), found);
}

}  // namespace

int dd_exact_screen_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* all,
                           const uint64_t* none, int nq, uint64_t* shared, uint64_t* match, uint64_t* found) {
    if (screen_args(c, fasta_dev, n, ns, k, all, none, nq, shared, match, found)) return DD_EINVAL;
    if (universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = universe_prepare(c, fasta_dev, nbytes, n, ns, in))) return rc;
    size_t sample_segments = 0;
    for (int g = n; g < n + ns; ++g) sample_segments = std::max(sample_segments, (nbytes[g] + dd::kSegTokens - 1) / dd::kSegTokens);
    const size_t rows = (size_t)ns + 1, ncount = rows * ((size_t)n + (size_t)nq);
    std::vector<unsigned long long> host(ncount, 0ull);
    ExactRecords rec;
    if (in.slots) {
        std::vector<char> image(kOwnTable + sizeof(uint64_t) * 2 * (size_t)nq, 0);   // the caller's (all, none) [nq][2]
        uint64_t* pairs = static_cast<uint64_t*>(own_table(image.data()));
        for (int q = 0; q < nq; ++q) pairs[2 * q] = all[q], pairs[2 * q + 1] = none[q];
        if ((rc = exact_records(c, in, n, k, "exact screen", &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec))) return rc;
    }
    if (rec.kept) {
        // counters [ns + 1][n] | [ns + 1][nq], then the seen bitmaps [ns][words]
        const size_t words = ((size_t)rec.found + 31) / 32, cbytes = align_up(ncount * sizeof(unsigned long long), 256),
                     sbytes = (size_t)ns * words * sizeof(uint32_t);
        if (c->hits.reserve(cbytes + sbytes))
            return fail(DD_ENOMEM, "exact screen: no device memory for the %zu bytes of the samples' seen bitmaps (%d samples x %zu words of 32 records)",
                        sbytes, ns, words);
        unsigned long long* shared_dev = static_cast<unsigned long long*>(c->hits.p);
        unsigned long long* match_dev = shared_dev + rows * (size_t)n;
        uint32_t* seen_dev = reinterpret_cast<uint32_t*>(static_cast<char*>(c->hits.p) + cbytes);
        DD_HIP(hipMemsetAsync(c->hits.p, 0, cbytes + sbytes, st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};
            DD_HIP(rec.order(c, k, &set));
            dd::launch_exact_screen(in.etab_dev + n, ns, sample_segments, k, c->canonical, set, seen_dev, words, st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_tally(set, seen_dev, words, ns, n, nq, static_cast<const uint64_t*>(own_table(c->ord.p)), shared_dev, match_dev, st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(host.data(), shared_dev, ncount * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
    }
    // (nothing is written before everything is known)
    for (size_t i = 0; i < rows * (size_t)n; ++i) shared[i] = host[i];
    for (size_t i = 0; i < rows * (size_t)nq; ++i) match[i] = host[rows * (size_t)n + i];
    *found = rec.found;
    return DD_OK;
}

int dd_exact_screen(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const uint64_t* all,
                    const uint64_t* none, int nq, uint64_t* shared, uint64_t* match, uint64_t* found) {
    if (screen_args(c, paths, n, ns, k, all, none, nq, shared, match, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_screen_device(c, p, s, n, ns, k, all, none, nq, shared, match, found);
    });
}

// ------------------------------------------------------------------- samples painted window by window
// dd_exact_paint.hip: the records of the universe put in key order, then one walk of every sample that keeps the position: a
// row of n + 2 counters per window of the sample's token stream, in c->hits.  The shape of the answer is checked like
// dd_exact_locate's: each sample's share of off[] against its token count.
namespace {

// the rule of a window of tokens (paint: of a sample's stream; cover: of a target's)
int window_args(uint64_t window) {
    if (window < dd::kSegTokens || window > dd::kPaintMaxWindow || window % dd::kSegTokens)
        return fail(DD_EINVAL, "window=%llu: a multiple of %d in %d..%zu tokens (a window is whole 64-token segments)", (unsigned long long)window,
                    (int)dd::kSegTokens, (int)dd::kSegTokens, dd::kPaintMaxWindow);
    return DD_OK;
}

int paint_args(dd_ctx* c, const void* inputs, int n, int ns, int k, uint64_t window, const uint64_t* off, const uint64_t* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (window_args(window)) return DD_EINVAL;
    if (!off) return fail(DD_EINVAL, "null argument");
    return DD_OK;
}

}  // namespace

int dd_exact_paint_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, uint64_t window,
                          const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (paint_args(c, fasta_dev, n, ns, k, window, off, found)) return DD_EINVAL;
    if (universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (off[ns] < off[0]) return fail(DD_EINVAL, "off[] must ascend");
    const uint64_t rows = off[ns] - off[0];   // (each sample's own share is checked once the samples' token counts are known)
    if (rows && !counts) return fail(DD_EINVAL, "null argument");
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = universe_prepare(c, fasta_dev, nbytes, n, ns, in))) return rc;
    std::vector<unsigned long long> ntok;   // the shape of the answer: every sample's ntok
    if ((rc = exact_read_ntok(c, in, n, ns, ntok))) return rc;
    std::vector<char> image(kOwnTable + sizeof(unsigned long long) * (size_t)ns, 0);   // the first row of every sample [ns]
    unsigned long long* row0 = static_cast<unsigned long long*>(own_table(image.data()));
    size_t sample_segments = 0;
    for (int s = 0; s < ns; ++s) {
        const uint64_t want = (ntok[(size_t)s] + window - 1) / window;
        if (off[s + 1] - off[s] != want)
            return fail(DD_EINVAL, "sample %d: off[%d] - off[%d] = %llu rows, %llu expected (it holds %llu tokens, %llu to a window)", s, s + 1, s,
                        (unsigned long long)(off[s + 1] - off[s]), (unsigned long long)want, ntok[(size_t)s], (unsigned long long)window);
        row0[s] = off[s] - off[0];
        sample_segments = std::max(sample_segments, (size_t)((ntok[(size_t)s] + dd::kSegTokens - 1) / dd::kSegTokens));
    }
    const size_t ncol = (size_t)n + 2, cbytes = (size_t)rows * ncol * sizeof(uint32_t);
    ExactRecords rec;
    if (in.slots) {
        if ((rc = exact_records(c, in, n, k, "exact paint", &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec))) return rc;
    } else if (rows) {
        if ((rc = stage_table(c, c->ord, image.data(), image.size()))) return rc;   // (no emission has staged it)
    }
    std::vector<uint32_t> host((size_t)rows * ncol);
    if (rows) {
        if (c->hits.reserve(cbytes))
            return fail(DD_ENOMEM, "exact paint: no device memory for the %zu bytes of the windows' counters (%llu rows x %zu columns of 4 bytes)",
                        cbytes, (unsigned long long)rows, ncol);
        uint32_t* counts_dev = static_cast<uint32_t*>(c->hits.p);
        DD_HIP(hipMemsetAsync(counts_dev, 0, cbytes, st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};   // (an empty universe: no record, column 0 alone)
            if (rec.kept) DD_HIP(rec.order(c, k, &set));
            dd::launch_exact_paint(in.etab_dev + n, ns, sample_segments, k, c->canonical, set, n, (size_t)(window / dd::kSegTokens),
                                   static_cast<const unsigned long long*>(own_table(c->ord.p)), counts_dev, st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(host.data(), counts_dev, cbytes, hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        memcpy(counts + off[0] * ncol, host.data(), cbytes);   // (nothing is written before everything is known)
    }
    *found = rec.found;
    return DD_OK;
}

int dd_exact_paint(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, uint64_t window,
                   const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (paint_args(c, paths, n, ns, k, window, off, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_paint_device(c, p, s, n, ns, k, window, off, counts, found);
    });
}

// ------------------------------------------------------------------- samples called row by row
// dd_exact_reads.hip: paint's frame with the caller's borders for rows -- the records of a read set or of a draft assembly,
// or any intervals -- then the vote over every row's counters and the tally of the votes per sample, all in c->hits:
// counters [rows][n + 2] u32 | borders [rows] u64 | calls [rows][6] u32 | sets [rows][2] u64 | tally [ns][n + 3] u64, the
// call arrays only where the caller takes them.  The borders are checked against the samples' token counts on the host.
namespace {

int reads_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* off, const uint64_t* start, uint32_t min_hits,
               const uint64_t* tally, const uint64_t* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (!min_hits) return fail(DD_EINVAL, "min_hits=0: a call needs at least one position of its genome (min_hits >= 1)");
    if (!off || !tally) return fail(DD_EINVAL, "null argument");
    for (int s = 0; s < ns; ++s)
        if (off[s + 1] < off[s]) return fail(DD_EINVAL, "off[] must ascend");
    if (off[ns] > off[0] && !start) return fail(DD_EINVAL, "null argument");
    return DD_OK;
}

}  // namespace

int dd_exact_reads_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* off,
                          const uint64_t* start, uint32_t min_hits, uint32_t* calls, uint64_t* sets, uint32_t* counts, uint64_t* tally,
                          uint64_t* found) {
    if (reads_args(c, fasta_dev, n, ns, k, off, start, min_hits, tally, found)) return DD_EINVAL;
    if (universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    const uint64_t rows = off[ns] - off[0];
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = universe_prepare(c, fasta_dev, nbytes, n, ns, in))) return rc;
    std::vector<unsigned long long> ntok;   // what the borders are checked against: every sample's ntok
    if ((rc = exact_read_ntok(c, in, n, ns, ntok))) return rc;
    std::vector<char> image(kOwnTable + sizeof(unsigned long long) * ((size_t)ns + 1), 0);   // the first row of every sample, and the end [ns + 1]
    unsigned long long* off0 = static_cast<unsigned long long*>(own_table(image.data()));
    size_t sample_segments = 0, sample_rows = 0;
    for (int s = 0; s < ns; ++s) {
        for (uint64_t r = off[s]; r < off[s + 1]; ++r) {
            if (r > off[s] && start[r] <= start[r - 1])
                return fail(DD_EINVAL, "sample %d, row %llu: start = %llu does not ascend strictly (the row in front starts at %llu)", s,
                            (unsigned long long)(r - off[s]), (unsigned long long)start[r], (unsigned long long)start[r - 1]);
            if (start[r] > ntok[(size_t)s])
                return fail(DD_EINVAL, "sample %d, row %llu: start = %llu lies behind the sample's %llu tokens", s, (unsigned long long)(r - off[s]),
                            (unsigned long long)start[r], ntok[(size_t)s]);
        }
        off0[s] = off[s] - off[0], off0[s + 1] = off[s + 1] - off[0];
        sample_rows = std::max(sample_rows, (size_t)(off[s + 1] - off[s]));
        if (off[s + 1] > off[s]) sample_segments = std::max(sample_segments, (size_t)((ntok[(size_t)s] + dd::kSegTokens - 1) / dd::kSegTokens));
    }
    const size_t ncol = (size_t)n + 2, nbin = (size_t)n + 3;
    const size_t cbytes = align_up((size_t)rows * ncol * sizeof(uint32_t), 256), bbytes = align_up((size_t)rows * sizeof(uint64_t), 256),
                 lbytes = calls ? align_up((size_t)rows * 6 * sizeof(uint32_t), 256) : 0,
                 sbytes = sets ? align_up((size_t)rows * 2 * sizeof(uint64_t), 256) : 0, tbytes = (size_t)ns * nbin * sizeof(uint64_t);
    ExactRecords rec;
    if (in.slots) {
        if ((rc = exact_records(c, in, n, k, "exact reads", &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec))) return rc;
    } else if (rows) {
        if ((rc = stage_table(c, c->ord, image.data(), image.size()))) return rc;   // (no emission has staged it)
    }
    std::vector<uint64_t> tally_host((size_t)ns * nbin, 0);
    std::vector<uint32_t> calls_host(calls ? (size_t)rows * 6 : 0), counts_host(counts ? (size_t)rows * ncol : 0);
    std::vector<uint64_t> sets_host(sets ? (size_t)rows * 2 : 0);
    if (rows) {
        const size_t total = cbytes + bbytes + lbytes + sbytes + tbytes;
        if (c->hits.reserve(total))
            return fail(DD_ENOMEM, "exact reads: no device memory for the %zu bytes of the rows (%llu rows: %zu of counters, %zu columns of 4 bytes, %zu of "
                                   "borders, %zu of calls and sets) and of the tally",
                        total, (unsigned long long)rows, cbytes, ncol, bbytes, lbytes + sbytes);
        char* base = static_cast<char*>(c->hits.p);
        uint32_t* counts_dev = reinterpret_cast<uint32_t*>(base);
        unsigned long long* start_dev = reinterpret_cast<unsigned long long*>(base + cbytes);
        uint32_t* calls_dev = calls ? reinterpret_cast<uint32_t*>(base + cbytes + bbytes) : nullptr;
        uint64_t* sets_dev = sets ? reinterpret_cast<uint64_t*>(base + cbytes + bbytes + lbytes) : nullptr;
        unsigned long long* tally_dev = reinterpret_cast<unsigned long long*>(base + cbytes + bbytes + lbytes + sbytes);
        DD_HIP(hipMemsetAsync(counts_dev, 0, cbytes, st));
        DD_HIP(hipMemsetAsync(tally_dev, 0, tbytes, st));
        DD_HIP(hipMemcpyAsync(start_dev, start + off[0], (size_t)rows * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};   // (an empty universe: no record, column 0 alone)
            if (rec.kept) DD_HIP(rec.order(c, k, &set));
            const unsigned long long* off_dev = static_cast<const unsigned long long*>(own_table(c->ord.p));
            dd::launch_exact_reads(in.etab_dev + n, ns, sample_segments, k, c->canonical, set, n, off_dev, start_dev, counts_dev, st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_vote(counts_dev, off_dev, ns, sample_rows, n, min_hits, calls_dev, sets_dev, tally_dev, st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(tally_host.data(), tally_dev, tbytes, hipMemcpyDeviceToHost, st));
        if (calls) DD_HIP(hipMemcpyAsync(calls_host.data(), calls_dev, calls_host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (sets) DD_HIP(hipMemcpyAsync(sets_host.data(), sets_dev, sets_host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (counts) DD_HIP(hipMemcpyAsync(counts_host.data(), counts_dev, counts_host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
    }
    // (nothing is written before everything is known)
    if (calls && rows) memcpy(calls + off[0] * 6, calls_host.data(), calls_host.size() * sizeof(uint32_t));
    if (sets && rows) memcpy(sets + off[0] * 2, sets_host.data(), sets_host.size() * sizeof(uint64_t));
    if (counts && rows) memcpy(counts + off[0] * ncol, counts_host.data(), counts_host.size() * sizeof(uint32_t));
    memcpy(tally, tally_host.data(), tally_host.size() * sizeof(uint64_t));
    *found = rec.found;
    return DD_OK;
}

int dd_exact_reads(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const uint64_t* off,
                   const uint64_t* start, uint32_t min_hits, uint32_t* calls, uint64_t* sets, uint32_t* counts, uint64_t* tally,
                   uint64_t* found) {
    if (reads_args(c, paths, n, ns, k, off, start, min_hits, tally, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_reads_device(c, p, s, n, ns, k, off, start, min_hits, calls, sets, counts, tally, found);
    });
}

// ------------------------------------------------------------------- samples counted record by record
// dd_exact_depth.hip: screen's frame with a 32-bit counter per (sample, record) where screen keeps a bit, and a tally that
// bins the counters by depth.  The universe is sorted, emitted, ordered and its rows sized (launch_exact_tally without a
// sample: |G_i| and every query class) once per call; the samples are then taken in ROUNDS of as many counter rows as
// DD_DEPTH_MB holds, each round a memset, the walk and the tally.  c->hits: sizes [n + nq] u64 | per round hist
// [per][n + nq][bins] u64 | overflow [per][n + nq] u64 | counters [per][found] u32.
namespace {

int depth_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* all, const uint64_t* none, int nq, int bins,
               const uint64_t* hist, const uint64_t* total, const uint64_t* found) {
    if (universe_query_args(c, inputs, n, ns, k, all, none, nq, !hist || !total, found)) return DD_EINVAL;
    if (bins < 2 || bins > dd::kDepthMaxBins)
        return fail(DD_EINVAL, "bins=%d outside 2..%d: bin 0, then at least the clipped bin (depth >= bins - 1)", bins, dd::kDepthMaxBins);
    return DD_OK;
}

// a counter of depth_kernel holds the positions of one sample, which are fewer than its bytes (depth, cover)
int depth_sample_bytes(const size_t* nbytes, int n, int ns) {
    for (int g = n; g < n + ns; ++g)
        if ((unsigned long long)nbytes[g] >> 32)
            return fail(DD_EINVAL, "sample %d: %zu bytes, a sample must stay below 2^32 bytes (a record's depth is a 32-bit counter); split it over calls",
                        g - n, nbytes[g]);
    return DD_OK;
}

}  // namespace

int dd_exact_depth_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* all,
                          const uint64_t* none, int nq, int bins, uint64_t* hist, uint64_t* total, uint64_t* found) {
    if (depth_args(c, fasta_dev, n, ns, k, all, none, nq, bins, hist, total, found)) return DD_EINVAL;
    if (universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (depth_sample_bytes(nbytes, n, ns)) return DD_EINVAL;
    const size_t budget = exact_budget("DD_DEPTH_MB", (size_t)8 << 30);
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = universe_prepare(c, fasta_dev, nbytes, n, ns, in))) return rc;
    const size_t nrow = (size_t)n + (size_t)nq, B = (size_t)bins;
    std::vector<unsigned long long> hist_host((size_t)ns * nrow * B, 0ull), over_host((size_t)ns * nrow, 0ull), size_host(nrow, 0ull);
    ExactRecords rec;
    if (in.slots) {
        std::vector<char> image(kOwnTable + sizeof(uint64_t) * 2 * (size_t)nq, 0);   // the caller's (all, none) [nq][2]
        uint64_t* pairs = static_cast<uint64_t*>(own_table(image.data()));
        for (int q = 0; q < nq; ++q) pairs[2 * q] = all[q], pairs[2 * q + 1] = none[q];
        if ((rc = exact_records(c, in, n, k, "exact depth", &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec))) return rc;
    }
    if (rec.kept) {
        // a round's row: the sample's counters and its histograms
        const size_t fnd = (size_t)rec.found, row_bytes = fnd * sizeof(uint32_t) + nrow * (B + 1) * sizeof(unsigned long long);
        if (budget < row_bytes)
            return fail(DD_ENOMEM, "exact depth: one sample needs %zu bytes of counters (%zu records x 4 bytes, and %zu rows x %d bins x 8), "
                                   "DD_DEPTH_MB holds %zu MiB now",
                        row_bytes, fnd, nrow, bins, budget >> 20);
        const size_t per = std::min((size_t)ns, budget / row_bytes);
        const size_t zbytes = align_up(nrow * sizeof(unsigned long long), 256), hbytes = align_up(per * nrow * B * sizeof(unsigned long long), 256),
                     obytes = align_up(per * nrow * sizeof(unsigned long long), 256), cbytes = per * fnd * sizeof(uint32_t);
        if (c->hits.reserve(zbytes + hbytes + obytes + cbytes))
            return fail(DD_ENOMEM, "exact depth: no device memory for the %zu bytes of a round's counters (%zu samples x %zu records x 4 bytes) and the "
                                   "%zu of its histograms; a smaller DD_DEPTH_MB (%zu MiB now) makes smaller rounds",
                        cbytes, per, fnd, hbytes + obytes, budget >> 20);
        char* base = static_cast<char*>(c->hits.p);
        unsigned long long* size_dev = reinterpret_cast<unsigned long long*>(base);
        unsigned long long* hist_dev = reinterpret_cast<unsigned long long*>(base + zbytes);
        unsigned long long* over_dev = reinterpret_cast<unsigned long long*>(base + zbytes + hbytes);
        uint32_t* count_dev = reinterpret_cast<uint32_t*>(base + zbytes + hbytes + obytes);
        const uint64_t* table_dev = static_cast<const uint64_t*>(own_table(c->ord.p));
        DD_HIP(hipMemsetAsync(size_dev, 0, zbytes, st));
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(rec.order(c, k, &set));
        dd::launch_exact_tally(set, nullptr, 0, 0, n, nq, table_dev, size_dev, size_dev + n, st);   // (no sample: the universe's row alone)
        DD_HIP(hipGetLastError());
        DD_HIP(hipMemcpyAsync(size_host.data(), size_dev, nrow * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        for (size_t s0 = 0; s0 < (size_t)ns; s0 += per) {
            const size_t take = std::min(per, (size_t)ns - s0);
            size_t sample_segments = 0;
            for (size_t s = s0; s < s0 + take; ++s)
                sample_segments = std::max(sample_segments, (nbytes[(size_t)n + s] + dd::kSegTokens - 1) / dd::kSegTokens);
            DD_HIP(hipMemsetAsync(hist_dev, 0, hbytes + obytes + take * fnd * sizeof(uint32_t), st));
            dd::launch_exact_depth(in.etab_dev + n + s0, (int)take, sample_segments, k, c->canonical, set, count_dev, st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_depth_tally(set, count_dev, (int)take, n, nq, bins, table_dev, hist_dev, over_dev, st);
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(hist_host.data() + s0 * nrow * B, hist_dev, take * nrow * B * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            DD_HIP(hipMemcpyAsync(over_host.data() + s0 * nrow, over_dev, take * nrow * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));   // (the next round clears what these copies read)
        }
    }
    // bin 0: the row's records less those the sample holds; the total from the bins and the clipped records' overflow
    // (nothing is written before everything is known)
    for (size_t s = 0; s < (size_t)ns; ++s)
        for (size_t r = 0; r < nrow; ++r) {
            unsigned long long* h = hist_host.data() + (s * nrow + r) * B;
            unsigned long long held = 0, sum = over_host[s * nrow + r];
            for (size_t d = 1; d < B; ++d) held += h[d], sum += d * h[d];
            h[0] = size_host[r] - held;
            total[s * nrow + r] = sum;
        }
    for (size_t i = 0; i < hist_host.size(); ++i) hist[i] = hist_host[i];
    *found = rec.found;
    return DD_OK;
}

int dd_exact_depth(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const uint64_t* all,
                   const uint64_t* none, int nq, int bins, uint64_t* hist, uint64_t* total, uint64_t* found) {
    if (depth_args(c, paths, n, ns, k, all, none, nq, bins, hist, total, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_depth_device(c, p, s, n, ns, k, all, none, nq, bins, hist, total, found);
    });
}

// ------------------------------------------------------------------- samples laid along the genomes of the universe
// dd_exact_cover.hip: depth's frame -- the universe sorted, emitted and ordered once per call, the samples in rounds under
// DD_DEPTH_MB, each round a memset and depth_kernel as it is -- with the record of every target position looked up ONCE, in
// front of the rounds, and a kernel per round that gathers the round's counters through that index into window rows.  The
// shape of the answer is checked like dd_exact_paint's: each target's share of off[] against its token count.
// c->hits: index [the targets' token slots] u32 | per round rows [per][off[nt] - off[0]][6] u32 | counters [per][found] u32.
namespace {

int cover_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const int32_t* target, int nt, uint64_t window, uint32_t clip,
               const uint64_t* off, const uint64_t* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (nt < 1 || nt > n) return fail(DD_EINVAL, "nt=%d outside 1..%d: the targets are inputs of the universe, each once", nt, n);
    if (!target || !off) return fail(DD_EINVAL, "null argument");
    uint64_t seen = 0;
    for (int t = 0; t < nt; ++t) {
        if (target[t] < 0 || target[t] >= n) return fail(DD_EINVAL, "target %d: input %d outside 0..%d", t, target[t], n - 1);
        if (seen >> target[t] & 1ull) {
            int first = 0;
            while (target[first] != target[t]) ++first;
            return fail(DD_EINVAL, "target %d: input %d is target %d already (a target is laid out once)", t, target[t], first);
        }
        seen |= 1ull << target[t];
    }
    if (window_args(window)) return DD_EINVAL;
    if (clip < 1 || clip > dd::kCoverMaxClip)
        return fail(DD_EINVAL, "clip=%u outside 1..%u (a depth counts as min(depth, clip): a window's sum stays inside 32 bits)", clip, dd::kCoverMaxClip);
    for (int t = 0; t < nt; ++t)
        if (off[t + 1] < off[t]) return fail(DD_EINVAL, "off[] must ascend");
    return DD_OK;
}

}  // namespace

int dd_exact_cover_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const int32_t* target, int nt,
                          uint64_t window, uint32_t clip, const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (cover_args(c, fasta_dev, n, ns, k, target, nt, window, clip, off, found)) return DD_EINVAL;
    if (universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (depth_sample_bytes(nbytes, n, ns)) return DD_EINVAL;
    const uint64_t rows = off[nt] - off[0];   // of one sample (each target's own share is checked once the inputs' token counts are known)
    if (rows && !counts) return fail(DD_EINVAL, "null argument");
    const size_t budget = exact_budget("DD_DEPTH_MB", (size_t)8 << 30);
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = universe_prepare(c, fasta_dev, nbytes, n, ns, in))) return rc;
    std::vector<unsigned long long> ntok;   // the shape of the answer: every input's ntok
    if ((rc = exact_read_ntok(c, in, 0, n, ntok))) return rc;
    // the targets that hold a token, one launch unit each; the entry's own table
    std::vector<char> image(kOwnTable + sizeof(dd::CoverUnit) * (size_t)nt, 0);
    dd::CoverUnit* units = static_cast<dd::CoverUnit*>(own_table(image.data()));
    int nunits = 0;
    size_t target_segments = 0, words = 0;
    for (int t = 0; t < nt; ++t) {
        const unsigned long long tokens = ntok[(size_t)target[t]];
        const uint64_t want = (tokens + window - 1) / window;
        if (off[t + 1] - off[t] != want)
            return fail(DD_EINVAL, "target %d: off[%d] - off[%d] = %llu rows, %llu expected (input %d holds %llu tokens, %llu to a window)", t, t + 1, t,
                        (unsigned long long)(off[t + 1] - off[t]), (unsigned long long)want, target[t], tokens, (unsigned long long)window);
        if (!tokens) continue;   // (it owns no row)
        const dd::ExactGenome& eg = in.etab[(size_t)target[t]];
        const size_t segs = (size_t)((tokens + dd::kSegTokens - 1) / dd::kSegTokens);
        dd::CoverUnit& u = units[nunits++];
        u.codes = eg.codes, u.bad = eg.bad, u.ntok = eg.ntok, u.index = words, u.row0 = off[t] - off[0], u.genome = target[t];
        words += segs * dd::kSegTokens, target_segments = std::max(target_segments, segs);
    }
    ExactRecords rec;
    if (in.slots) {
        if ((rc = exact_records(c, in, n, k, "exact cover", &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec))) return rc;
    }
    if (rec.found >> 31)
        return fail(DD_EINVAL, "exact cover: the universe holds %llu distinct k-mers, a position's index word holds a record below 2^31 (and the "
                               "private flag); lay the samples along a smaller universe",
                    rec.found);
    const size_t R = (size_t)rows, row_words = R * dd::kCoverColumns;
    std::vector<uint32_t> host((size_t)ns * row_words, 0u);
    if (rec.kept && R) {
        // a round's row: the sample's counters and its windows
        const size_t fnd = (size_t)rec.found, ibytes = align_up(words * sizeof(uint32_t), 256),
                     row_bytes = fnd * sizeof(uint32_t) + row_words * sizeof(uint32_t);
        if (budget < row_bytes)
            return fail(DD_ENOMEM, "exact cover: one sample needs %zu bytes (%zu records x 4 bytes of counters, and %zu windows x %d columns x 4), "
                                   "DD_DEPTH_MB holds %zu MiB now",
                        row_bytes, fnd, R, dd::kCoverColumns, budget >> 20);
        const size_t per = std::min((size_t)ns, budget / row_bytes);
        const size_t wbytes = align_up(per * row_words * sizeof(uint32_t), 256), cbytes = per * fnd * sizeof(uint32_t);
        if (c->hits.reserve(ibytes + wbytes + cbytes))
            return fail(DD_ENOMEM, "exact cover: no device memory for the %zu bytes of the targets' index (%zu token slots x 4 bytes), the %zu of a round's "
                                   "counters (%zu samples x %zu records x 4 bytes) and the %zu of its windows; a smaller DD_DEPTH_MB (%zu MiB now) makes "
                                   "smaller rounds",
                        ibytes, words, cbytes, per, fnd, wbytes, budget >> 20);
        char* base = static_cast<char*>(c->hits.p);
        uint32_t* index_dev = reinterpret_cast<uint32_t*>(base);
        uint32_t* rows_dev = reinterpret_cast<uint32_t*>(base + ibytes);
        uint32_t* count_dev = reinterpret_cast<uint32_t*>(base + ibytes + wbytes);
        const dd::CoverUnit* units_dev = static_cast<const dd::CoverUnit*>(own_table(c->ord.p));
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(rec.order(c, k, &set));
        dd::launch_exact_cover_index(units_dev, nunits, target_segments, k, c->canonical, set, index_dev, st);
        DD_HIP(hipGetLastError());
        for (size_t s0 = 0; s0 < (size_t)ns; s0 += per) {
            const size_t take = std::min(per, (size_t)ns - s0);
            size_t sample_segments = 0;
            for (size_t s = s0; s < s0 + take; ++s)
                sample_segments = std::max(sample_segments, (nbytes[(size_t)n + s] + dd::kSegTokens - 1) / dd::kSegTokens);
            DD_HIP(hipMemsetAsync(rows_dev, 0, wbytes + take * fnd * sizeof(uint32_t), st));
            dd::launch_exact_depth(in.etab_dev + n + s0, (int)take, sample_segments, k, c->canonical, set, count_dev, st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_cover(units_dev, nunits, target_segments, index_dev, count_dev, fnd, (int)take, (size_t)(window / dd::kSegTokens), clip, R,
                                   rows_dev, st);
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(host.data() + s0 * row_words, rows_dev, take * row_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));   // (the next round clears what this copy reads)
        }
    }
    // sample s owns counts[s][off[0] .. off[nt]-1] of its off[nt] rows (nothing is written before everything is known)
    for (size_t s = 0; s < (size_t)ns && R; ++s)
        memcpy(counts + (s * (size_t)off[nt] + (size_t)off[0]) * dd::kCoverColumns, host.data() + s * row_words, row_words * sizeof(uint32_t));
    *found = rec.found;
    return DD_OK;
}

int dd_exact_cover(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const int32_t* target, int nt,
                   uint64_t window, uint32_t clip, const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (cover_args(c, paths, n, ns, k, target, nt, window, clip, off, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_cover_device(c, p, s, n, ns, k, target, nt, window, clip, off, counts, found);
    });
}

// ------------------------------------------------------------------- the membership-pattern table
// dd_exact_sched.hip's patterns accumulator behind the sort of the schedules for ONE k: a pass leaves (mask, count) pairs in
// the pair area of the workspace (sized for one pair per slot of the pass, which no pass can exceed), dd_exact_patterns.hip
// sorts and reduces them in the k-mer arrays the schedule has consumed and merges the rows into the running table, which
// lives in c->pat[cur] and moves to the other buffer with every merge.  Behind the last pass the table is put in answer
// order in the workspace and its first min(found, cap) rows come back.
namespace {

int pattern_slots(int* slots) {
    *slots = dd::kPatternSlotsDefault;
    if (const char* e = getenv("DD_PATTERNS_SLOTS")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end || v < dd::kPatternSlotsMin || v > dd::kPatternSlotsMax || (v & (v - 1)))
            return fail(DD_EINVAL, "DD_PATTERNS_SLOTS=%s: a power of two in %d..%d (the slots of a workgroup's table in LDS)", e,
                        dd::kPatternSlotsMin, dd::kPatternSlotsMax);
        *slots = (int)v;
    }
    return DD_OK;
}

}  // namespace

int dd_exact_patterns_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k, uint64_t* masks,
                             uint64_t* counts, size_t cap, uint64_t* found, uint64_t* stats) {
    if (exact_frame(c, fasta_dev, nbytes, n, 64, k, k, found, cap && (!masks || !counts))) return DD_EINVAL;
    int slots = 0;
    if (pattern_slots(&slots)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    *found = 0;
    unsigned long long tally[4] = {0, 0, 0, 0};   // the stats of the ABI
    const auto done = [&] {
        for (int i = 0; stats && i < 4; ++i) stats[i] = tally[i];
        return DD_OK;
    };
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    c->st_blocks = 0;
    if (!in.slots) return done();
    if ((rc = c->hist.reserve(sizeof(unsigned long long)))) return rc;
    unsigned long long* seen_dev = static_cast<unsigned long long*>(c->hist.p);   // M, over all passes
    DD_HIP(hipMemsetAsync(seen_dev, 0, sizeof(unsigned long long), st));
    // the running table: rows in mask order, in c->pat[cur]
    int cur = 0;
    size_t rows = 0;
    const uint64_t* tab_mask = nullptr;
    const unsigned long long* tab_count = nullptr;
    const ExactLayout layout{"exact patterns", dd::exact_tag_mode(k), dd::exact_patterns_temp_bytes, dd::exact_patterns_scratch_bytes};
    rc = exact_passes(c, in, n, k, layout, [&](const ExactArrays& a, size_t count) -> int {
        dd::ExactSorted sorted{};
        DD_HIP(dd::launch_exact_sort_tagged(a.lo, a.hi, a.lo_alt, a.hi_alt, a.g, a.g_alt, count, k, a.temp, a.temp_bytes, st, &sorted));
        // (the workspace was carved for at least `count` slots, and every part of the scratch grows with them)
        const dd::PatternPairs pp = dd::exact_patterns_pairs(a.scratch, count);
        DD_HIP(hipMemsetAsync(pp.head, 0, 256, st));
        dd::ExactSched s{dd::kSchedPatterns, n, slots, 0, nullptr, seen_dev};
        s.store = pp.mask, s.counts = pp.count, s.cursor = pp.head, s.overflow = pp.head + 1, s.pstats = pp.head + 2, s.cap = pp.cap;
        DD_HIP(dd::launch_exact_sched(sorted, count, k, s, pp.sched_scratch, st));
        unsigned long long h[5] = {0, 0, 0, 0, 0};   // cursor, overflow, forced flushes, single masks, rows of the reduce
        DD_HIP(hipMemcpyAsync(h, pp.head, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        if (h[1] || h[0] > pp.cap)
            return fail(DD_EHIP, "exact patterns: a pass of %zu k-mer slots wrote %llu pairs, one per distinct k-mer at the most was expected", count, h[0]);
        tally[1] += h[0], tally[2] += h[2], tally[3] += h[3];
        if (!h[0]) return DD_OK;
        // the k-mers are consumed: their arrays are the sort's other half
        DD_HIP(dd::launch_patterns_reduce(pp, (size_t)h[0], n, a.lo, reinterpret_cast<unsigned long long*>(a.lo_alt), a.temp, a.temp_bytes, st));
        DD_HIP(hipMemcpyAsync(h + 4, pp.head + 4, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        const size_t fresh = (size_t)h[4], bytes = dd::exact_patterns_merge_bytes(rows + fresh);
        DevBuf& dst = c->pat[cur ^ 1];
        if (dst.reserve(bytes))
            return fail(DD_ENOMEM, "exact patterns: no device memory for the %zu bytes that merge %zu rows into a table of %zu", bytes, fresh, rows);
        unsigned long long* rows_dev = nullptr;
        DD_HIP(dd::launch_patterns_merge(tab_mask, tab_count, rows, pp.mask, pp.count, fresh, dst.p, &rows_dev, st));
        DD_HIP(hipMemcpyAsync(h + 4, rows_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        tab_mask = static_cast<const uint64_t*>(dst.p);
        tab_count = reinterpret_cast<const unsigned long long*>(static_cast<const char*>(dst.p) + dd::exact_patterns_stride(rows + fresh));
        rows = (size_t)h[4], cur ^= 1;
        return DD_OK;
    });
    if (rc) return rc;
    DD_HIP(hipMemcpyAsync(&tally[0], seen_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    const size_t take = std::min(rows, cap);
    if (take) {
        const size_t bytes = dd::exact_patterns_order_bytes(rows);
        if (c->exact.reserve(bytes)) return fail(DD_ENOMEM, "exact patterns: no device memory for the %zu bytes that put %zu rows in order", bytes, rows);
        {
            Span sp(c, DD_KERNEL_EXACT);
            DD_HIP(dd::launch_patterns_order(tab_mask, tab_count, rows, c->exact.p, st));
        }
        std::vector<uint64_t> mk(take), inv(take);
        DD_HIP(hipMemcpyAsync(mk.data(), c->exact.p, take * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        DD_HIP(hipMemcpyAsync(inv.data(), static_cast<const char*>(c->exact.p) + dd::exact_patterns_stride(rows), take * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        for (size_t i = 0; i < take; ++i) masks[i] = mk[i], counts[i] = ~inv[i];   // (nothing is written before everything is known)
    }
    *found = rows;
    return done();
}

int dd_exact_patterns(dd_ctx* c, const char* const* paths, int n, int k, uint64_t* masks, uint64_t* counts, size_t cap, uint64_t* found,
                      uint64_t* stats) {
    return exact_path_form(c, paths, n, 64, k, k, found,
                           [&](auto p, auto s) { return dd_exact_patterns_device(c, p, s, n, k, masks, counts, cap, found, stats); });
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

}  // extern "C"
