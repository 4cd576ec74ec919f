// dd_exact_samples_api.hip -- the exact entry points of the C ABI (include/dandd_hip.h) that look SAMPLES, files that are no
// inputs, up in the ordered records of a universe of inputs: what the samples hold of them (dd_exact_screen), where along
// themselves (dd_exact_paint), which genome each of their records belongs to (dd_exact_reads), how many times they hold each
// (dd_exact_depth), where along each genome, and how deep (dd_exact_cover) and which genomes explain them, one by one
// (dd_exact_gather).  Each entry is its own argument rules, table and kernels (dd_exact_screen.hip, dd_exact_paint.hip,
// dd_exact_reads.hip, dd_exact_depth.hip, dd_exact_cover.hip, dd_exact_gather.hip) around
// four pieces: UniverseCall, HitsCarve, SampleRounds (below) and exact_check_shape (dd_exact_host.h).  It checks its
// arguments in the order of its ABI comment, stages every result on the host and writes the caller's arrays once, at its
// end: nothing is written before everything is known.  Host-side orchestration only.
#include "dd_exact_host.h"

namespace {

// ------------------------------------------------------------------- the argument rules the entries share
// the argument rules of the universe and the samples, in front of the entry's own ...
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

// ... and where depth_kernel counts (depth, cover): a counter holds the positions of one sample, which are fewer than its bytes
int depth_sample_bytes(const size_t* nbytes, int n, int ns) {
    for (int g = n; g < n + ns; ++g)
        if ((unsigned long long)nbytes[g] >> 32)
            return fail(DD_EINVAL, "sample %d: %zu bytes, a sample must stay below 2^32 bytes (a record's depth is a 32-bit counter); split it over calls",
                        g - n, nbytes[g]);
    return DD_OK;
}

// the rule of a window of tokens (paint: of a sample's stream; cover: of a target's)
int window_args(uint64_t window) {
    if (window < dd::kSegTokens || window > dd::kPaintMaxWindow || window % dd::kSegTokens)
        return fail(DD_EINVAL, "window=%llu: a multiple of %d in %d..%zu tokens (a window is whole 64-token segments)", (unsigned long long)window,
                    (int)dd::kSegTokens, (int)dd::kSegTokens, dd::kPaintMaxWindow);
    return DD_OK;
}

// ------------------------------------------------------------------- the entries' own argument rules, the same in both forms
int screen_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* all, const uint64_t* none, int nq,
                const uint64_t* shared, const uint64_t* match, const uint64_t* found) {
    return universe_query_args(c, inputs, n, ns, k, all, none, nq, !shared || (nq && !match), found);
}

int paint_args(dd_ctx* c, const void* inputs, int n, int ns, int k, uint64_t window, const uint64_t* off, const uint64_t* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (window_args(window)) return DD_EINVAL;
    if (!off) return fail(DD_EINVAL, "null argument");
    return DD_OK;
}

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

int depth_args(dd_ctx* c, const void* inputs, int n, int ns, int k, const uint64_t* all, const uint64_t* none, int nq, int bins,
               const uint64_t* hist, const uint64_t* total, const uint64_t* found) {
    if (universe_query_args(c, inputs, n, ns, k, all, none, nq, !hist || !total, found)) return DD_EINVAL;
    if (bins < 2 || bins > dd::kDepthMaxBins)
        return fail(DD_EINVAL, "bins=%d outside 2..%d: bin 0, then at least the clipped bin (depth >= bins - 1)", bins, dd::kDepthMaxBins);
    return DD_OK;
}

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

int gather_args(dd_ctx* c, const void* inputs, int n, int ns, int k, uint32_t min_hits, int steps, const int32_t* pick, const uint64_t* unique,
                const uint64_t* depth, const uint64_t* shared, const uint64_t* total, const uint64_t* found) {
    if (universe_args(c, inputs, n, ns, k, found)) return DD_EINVAL;
    if (!min_hits) return fail(DD_EINVAL, "min_hits=0: a pick needs at least one k-mer that no earlier pick holds (min_hits >= 1)");
    if (steps < 1 || steps > n) return fail(DD_EINVAL, "steps=%d outside 1..%d: a step picks an input of the universe, each at most once", steps, n);
    if (!pick || !unique || !depth || !shared || !total) return fail(DD_EINVAL, "null argument");
    return DD_OK;
}

// a path form behind the entry's argument rules: the universe's files and the samples read and uploaded as one list
int universe_path_form(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, const ExactDeviceForm& device_form) {
    if (!samples) return fail(DD_EINVAL, "null argument");
    std::vector<const char*> files((size_t)(n + ns));
    for (int i = 0; i < n + ns; ++i)
        if (!(files[(size_t)i] = i < n ? paths[i] : samples[i - n])) return fail(DD_EINVAL, "null argument");
    return exact_upload_files(c, files.data(), n + ns, device_form);
}

// ------------------------------------------------------------------- the universe and the samples
// the 64-token segments of a stream of so many tokens (or bytes: no stream holds more tokens than its file bytes), and the
// most among `count` streams: the x extent of a launch that walks them
size_t segments_of(unsigned long long tokens) { return (size_t)((tokens + dd::kSegTokens - 1) / dd::kSegTokens); }
size_t largest_segments(const size_t* nbytes, size_t count) {
    size_t most = 0;
    for (size_t i = 0; i < count; ++i) most = std::max(most, segments_of(nbytes[i]));
    return most;
}

// What every entry sets up, in the order it calls them.  K0 runs over the universe's n inputs AND the ns samples behind
// them, once.  The sort and the emission see the universe alone -- the samples stay out of the sort and out of the slot
// count that sizes the record area -- with the single query (0, 0); the entry's own table rides behind that query, kOwnTable
// bytes into the image on the host and into c->ord once it is staged.
constexpr size_t kOwnTable = 256;
struct UniverseCall {
    dd_ctx* c;
    DeviceGuard guard;
    hipStream_t st;
    int n, ns, k;
    const char* what;   // "exact screen": the entry in the messages
    ExactInputs in;
    ExactRecords rec;
    std::vector<char> image;
    size_t sample_segments = 0;   // of the largest sample whose tokens the entry has read (paint, reads; the others: largest_segments)
    UniverseCall(dd_ctx* c_, int n_, int ns_, int k_, const char* what_) : c(c_), guard(c_->device), st(c_->stream), n(n_), ns(ns_), k(k_), what(what_) {}

    // K0 over everything; then in.slots and in.max_segments are the universe's alone (in.slots = 0: it holds no token, nothing
    // is sorted), while in.etab still lists the samples behind the universe
    int prepare(const uint8_t* const* fasta_dev, const size_t* nbytes) {
        int rc;
        if ((rc = exact_prepare(c, fasta_dev, nbytes, n + ns, in))) return rc;
        c->st_blocks = 0;
        in.slots = 0, in.max_segments = 0;
        for (int g = 0; g < n; ++g) {
            const size_t segs = segments_of(nbytes[g]);
            in.slots += segs * dd::kSegTokens, in.max_segments = std::max(in.max_segments, segs);
        }
        return DD_OK;
    }
    const dd::ExactGenome* samples_dev(size_t first = 0) const { return in.etab_dev + n + first; }

    // the entry's own table: `count` zeroed T on the host, to be filled; then where it lies once staged
    template <class T> T* table(size_t count) { return image.assign(kOwnTable + sizeof(T) * count, 0), reinterpret_cast<T*>(image.data() + kOwnTable); }
    template <class T> const T* table_dev() const { return reinterpret_cast<const T*>(static_cast<const char*>(c->ord.p) + kOwnTable); }
    // ... the caller's (all, none) [nq][2] (screen, depth)
    void pairs(const uint64_t* all, const uint64_t* none, int nq) {
        uint64_t* t = table<uint64_t>(2 * (size_t)nq);
        for (int q = 0; q < nq; ++q) t[2 * q] = all[q], t[2 * q + 1] = none[q];
    }

    // Leaves the records of the universe in rec (found = 0, kept = false where it holds no token).  table_anyway: the entry
    // launches a kernel that reads its table even then (paint, reads: column 0 alone), so the table is staged without an emission.
    // rec.order() is the caller's to launch, inside its own timing span.
    int records(bool table_anyway) {
        if (in.slots) return exact_records(c, in, n, k, what, &kSlotsOfUniverse, 1, image.data(), image.size(), in.slots, rec);
        return table_anyway ? stage_table(c, c->ord, image.data(), image.size()) : DD_OK;
    }
    int done(uint64_t* found) const { return *found = rec.found, DD_OK; }
};

// ------------------------------------------------------------------- the parts of c->hits
// part<T>(count, aligned) declares the next part -- `count` T, padded to 256 bytes where `aligned` -- reserve() takes the sum,
// and carve(part) is the part's place in c->hits.  A part's `bytes` include its padding: what a memset over it clears.
template <class T> struct HitsPart { size_t at, bytes; };
struct HitsCarve {
    dd_ctx* c;
    size_t total = 0;
    explicit HitsCarve(dd_ctx* c_) : c(c_) {}
    template <class T> HitsPart<T> part(size_t count, bool aligned) {
        const HitsPart<T> p{total, aligned ? align_up(count * sizeof(T), 256) : count * sizeof(T)};
        total += p.bytes;
        return p;
    }
    int reserve() { return c->hits.reserve(total); }   // (the entry puts its own message over a refusal)
    template <class T> T* operator()(const HitsPart<T>& p) const { return reinterpret_cast<T*>(static_cast<char*>(c->hits.p) + p.at); }
};

// ------------------------------------------------------------------- the rounds of depth and cover
// The universe is sorted, emitted and ordered once per call; the samples are then taken in ROUNDS of `per` samples, as many
// as DD_DEPTH_MB holds of a round's rows: a sample's depth_kernel counters [found] u32 and what the entry's own kernel makes
// of them.  In c->hits the round's part is the entry's arrays, then the counters, and one memset clears both.
using SampleRound = std::function<int(size_t s0, size_t take)>;
struct SampleRounds {
    size_t budget = exact_budget("DD_DEPTH_MB", (size_t)8 << 30), per = 0;

    // per, from what one sample needs; `needs` says of what, in the refusal
    int size(const char* what, int ns, size_t row_bytes, const char* needs) {
        if (budget < row_bytes)
            return fail(DD_ENOMEM, "%s: one sample needs %zu bytes%s, DD_DEPTH_MB holds %zu MiB now", what, row_bytes, needs, budget >> 20);
        per = std::min((size_t)ns, budget / row_bytes);
        return DD_OK;
    }

    // Per round: the memset over the entry's `head_bytes` from `head` on and the counters of the round's samples behind them,
    // depth_kernel, then each(s0, take) -- the entry's kernel over the samples s0 .. s0 + take - 1 and its copies to the host.
    int run(const UniverseCall& u, const size_t* nbytes, const dd::LocateSet& set, void* head, size_t head_bytes, uint32_t* count_dev,
            const SampleRound& each) const {
        int rc;
        for (size_t s0 = 0; s0 < (size_t)u.ns; s0 += per) {
            const size_t take = std::min(per, (size_t)u.ns - s0);
            DD_HIP(hipMemsetAsync(head, 0, head_bytes + take * (size_t)u.rec.found * sizeof(uint32_t), u.st));
            dd::launch_exact_depth(u.samples_dev(s0), (int)take, largest_segments(nbytes + u.n + s0, take), u.k, u.c->canonical, set, count_dev, u.st);
            DD_HIP(hipGetLastError());
            if ((rc = each(s0, take))) return rc;
            DD_HIP(hipStreamSynchronize(u.st));   // (the next round clears what these copies read)
        }
        return DD_OK;
    }
};

}  // namespace

extern "C" {

// ------------------------------------------------------------------- samples screened against the universe
// dd_exact_screen.hip: the records of the universe put in key order, one walk of every sample that marks the records it
// holds, one tally of the marks.  The ordered set may lie in the exact workspace: no sort runs there before the tally has
// finished.  c->hits: counters [ns + 1][n] | [ns + 1][nq] u64 | the seen bitmaps [ns][words] u32.
int dd_exact_screen_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* all,
                           const uint64_t* none, int nq, uint64_t* shared, uint64_t* match, uint64_t* found) {
    if (screen_args(c, fasta_dev, n, ns, k, all, none, nq, shared, match, found) || universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    UniverseCall u(c, n, ns, k, "exact screen");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    const size_t rows = (size_t)ns + 1, ncount = rows * ((size_t)n + (size_t)nq);
    std::vector<unsigned long long> host(ncount, 0ull);
    u.pairs(all, none, nq);
    if ((rc = u.records(false))) return rc;
    if (u.rec.kept) {
        const size_t words = ((size_t)u.rec.found + 31) / 32;
        HitsCarve hits(c);
        const auto counters = hits.part<unsigned long long>(ncount, true);
        const auto seen = hits.part<uint32_t>((size_t)ns * words, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact screen: no device memory for the %zu bytes of the samples' seen bitmaps (%d samples x %zu words of 32 records)",
                        seen.bytes, ns, words);
        unsigned long long *shared_dev = hits(counters), *match_dev = shared_dev + rows * (size_t)n;
        uint32_t* seen_dev = hits(seen);
        DD_HIP(hipMemsetAsync(shared_dev, 0, hits.total, u.st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};
            DD_HIP(u.rec.order(c, k, &set));
            dd::launch_exact_screen(u.samples_dev(), ns, largest_segments(nbytes + n, (size_t)ns), k, c->canonical, set, seen_dev, words, u.st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_tally(set, seen_dev, words, ns, n, nq, u.table_dev<uint64_t>(), shared_dev, match_dev, u.st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(host.data(), shared_dev, ncount * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
        DD_HIP(hipStreamSynchronize(u.st));
    }
    for (size_t i = 0; i < rows * (size_t)n; ++i) shared[i] = host[i];
    for (size_t i = 0; i < rows * (size_t)nq; ++i) match[i] = host[rows * (size_t)n + i];
    return u.done(found);
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
// row of n + 2 counters per window of the sample's token stream.  The shape of the answer is checked like dd_exact_locate's:
// each sample's share of off[] against its token count.  c->hits: counters [off[ns] - off[0]][n + 2] u32.
int dd_exact_paint_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, uint64_t window,
                          const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (paint_args(c, fasta_dev, n, ns, k, window, off, found) || universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (off[ns] < off[0]) return fail(DD_EINVAL, "off[] must ascend");
    const uint64_t rows = off[ns] - off[0];   // (each sample's own share is checked once the samples' token counts are known)
    if (rows && !counts) return fail(DD_EINVAL, "null argument");
    UniverseCall u(c, n, ns, k, "exact paint");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    std::vector<unsigned long long> ntok;   // the shape of the answer: every sample's ntok
    if ((rc = exact_read_ntok(c, u.in, n, ns, ntok))) return rc;
    unsigned long long* row0 = u.table<unsigned long long>((size_t)ns);   // the first row of every sample [ns]
    const ExactShape shape{"sample", "rows", window, "window"};
    for (int s = 0; s < ns; ++s) {
        if (exact_check_shape(shape, s, off, -1, ntok[(size_t)s])) return DD_EINVAL;
        row0[s] = off[s] - off[0];
        u.sample_segments = std::max(u.sample_segments, segments_of(ntok[(size_t)s]));
    }
    if ((rc = u.records(rows != 0))) return rc;
    const size_t ncol = (size_t)n + 2;
    std::vector<uint32_t> host((size_t)rows * ncol);
    if (rows) {
        HitsCarve hits(c);
        const auto counters = hits.part<uint32_t>((size_t)rows * ncol, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact paint: no device memory for the %zu bytes of the windows' counters (%llu rows x %zu columns of 4 bytes)",
                        counters.bytes, (unsigned long long)rows, ncol);
        uint32_t* counts_dev = hits(counters);
        DD_HIP(hipMemsetAsync(counts_dev, 0, counters.bytes, u.st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};   // (an empty universe: no record, column 0 alone)
            if (u.rec.kept) DD_HIP(u.rec.order(c, k, &set));
            dd::launch_exact_paint(u.samples_dev(), ns, u.sample_segments, k, c->canonical, set, n, (size_t)(window / dd::kSegTokens),
                                   u.table_dev<unsigned long long>(), counts_dev, u.st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(host.data(), counts_dev, counters.bytes, hipMemcpyDeviceToHost, u.st));
        DD_HIP(hipStreamSynchronize(u.st));
        memcpy(counts + off[0] * ncol, host.data(), counters.bytes);
    }
    return u.done(found);
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
// or any intervals -- then the vote over every row's counters and the tally of the votes per sample.  The borders are checked
// against the samples' token counts on the host.  c->hits: counters [rows][n + 2] u32 | borders [rows] u64 | calls [rows][6]
// u32 | sets [rows][2] u64 | tally [ns][n + 3] u64, the call arrays only where the caller takes them.
int dd_exact_reads_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* off,
                          const uint64_t* start, uint32_t min_hits, uint32_t* calls, uint64_t* sets, uint32_t* counts, uint64_t* tally,
                          uint64_t* found) {
    if (reads_args(c, fasta_dev, n, ns, k, off, start, min_hits, tally, found) || universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    const uint64_t rows = off[ns] - off[0];
    UniverseCall u(c, n, ns, k, "exact reads");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    std::vector<unsigned long long> ntok;   // what the borders are checked against: every sample's ntok
    if ((rc = exact_read_ntok(c, u.in, n, ns, ntok))) return rc;
    unsigned long long* off0 = u.table<unsigned long long>((size_t)ns + 1);   // the first row of every sample, and the end [ns + 1]
    size_t sample_rows = 0;
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
        if (off[s + 1] > off[s]) u.sample_segments = std::max(u.sample_segments, segments_of(ntok[(size_t)s]));
    }
    if ((rc = u.records(rows != 0))) return rc;
    const size_t R = (size_t)rows, ncol = (size_t)n + 2, nbin = (size_t)n + 3;
    std::vector<uint64_t> tally_host((size_t)ns * nbin, 0);
    std::vector<uint32_t> calls_host(calls ? R * 6 : 0), counts_host(counts ? R * ncol : 0);
    std::vector<uint64_t> sets_host(sets ? R * 2 : 0);
    if (rows) {
        HitsCarve hits(c);
        const auto counters = hits.part<uint32_t>(R * ncol, true);
        const auto borders = hits.part<unsigned long long>(R, true);
        const auto called = hits.part<uint32_t>(calls_host.size(), true);
        const auto setted = hits.part<uint64_t>(sets_host.size(), true);
        const auto tallies = hits.part<unsigned long long>((size_t)ns * nbin, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact reads: no device memory for the %zu bytes of the rows (%llu rows: %zu of counters, %zu columns of 4 bytes, %zu of "
                                   "borders, %zu of calls and sets) and of the tally",
                        hits.total, (unsigned long long)rows, counters.bytes, ncol, borders.bytes, called.bytes + setted.bytes);
        uint32_t *counts_dev = hits(counters), *calls_dev = calls ? hits(called) : nullptr;
        uint64_t* sets_dev = sets ? hits(setted) : nullptr;
        unsigned long long *start_dev = hits(borders), *tally_dev = hits(tallies);
        DD_HIP(hipMemsetAsync(counts_dev, 0, counters.bytes, u.st));
        DD_HIP(hipMemsetAsync(tally_dev, 0, tallies.bytes, u.st));
        DD_HIP(hipMemcpyAsync(start_dev, start + off[0], R * sizeof(uint64_t), hipMemcpyHostToDevice, u.st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            dd::LocateSet set{};   // (an empty universe: no record, column 0 alone)
            if (u.rec.kept) DD_HIP(u.rec.order(c, k, &set));
            const unsigned long long* off_dev = u.table_dev<unsigned long long>();
            dd::launch_exact_reads(u.samples_dev(), ns, u.sample_segments, k, c->canonical, set, n, off_dev, start_dev, counts_dev, u.st);
            DD_HIP(hipGetLastError());
            dd::launch_exact_vote(counts_dev, off_dev, ns, sample_rows, n, min_hits, calls_dev, sets_dev, tally_dev, u.st);
            DD_HIP(hipGetLastError());
        }
        DD_HIP(hipMemcpyAsync(tally_host.data(), tally_dev, tallies.bytes, hipMemcpyDeviceToHost, u.st));
        if (calls) DD_HIP(hipMemcpyAsync(calls_host.data(), calls_dev, calls_host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, u.st));
        if (sets) DD_HIP(hipMemcpyAsync(sets_host.data(), sets_dev, sets_host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, u.st));
        if (counts) DD_HIP(hipMemcpyAsync(counts_host.data(), counts_dev, counts_host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, u.st));
        DD_HIP(hipStreamSynchronize(u.st));
    }
    if (calls && rows) memcpy(calls + off[0] * 6, calls_host.data(), calls_host.size() * sizeof(uint32_t));
    if (sets && rows) memcpy(sets + off[0] * 2, sets_host.data(), sets_host.size() * sizeof(uint64_t));
    if (counts && rows) memcpy(counts + off[0] * ncol, counts_host.data(), counts_host.size() * sizeof(uint32_t));
    memcpy(tally, tally_host.data(), tally_host.size() * sizeof(uint64_t));
    return u.done(found);
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
// bins the counters by depth.  The universe's rows are sized (launch_exact_tally without a sample: |G_i| and every query
// class) once per call, in front of the rounds; a round is the memset, depth_kernel and the tally.
// c->hits: sizes [n + nq] u64 | per round hist [per][n + nq][bins] u64 | overflow [per][n + nq] u64 | counters [per][found] u32.
int dd_exact_depth_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const uint64_t* all,
                          const uint64_t* none, int nq, int bins, uint64_t* hist, uint64_t* total, uint64_t* found) {
    if (depth_args(c, fasta_dev, n, ns, k, all, none, nq, bins, hist, total, found) || universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (depth_sample_bytes(nbytes, n, ns)) return DD_EINVAL;
    SampleRounds rounds;
    UniverseCall u(c, n, ns, k, "exact depth");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    const size_t nrow = (size_t)n + (size_t)nq, B = (size_t)bins;
    std::vector<unsigned long long> hist_host((size_t)ns * nrow * B, 0ull), over_host((size_t)ns * nrow, 0ull), size_host(nrow, 0ull);
    u.pairs(all, none, nq);
    if ((rc = u.records(false))) return rc;
    if (u.rec.kept) {
        // a round's row: the sample's counters and its histograms
        const size_t fnd = (size_t)u.rec.found;
        char needs[160];
        snprintf(needs, sizeof needs, " of counters (%zu records x 4 bytes, and %zu rows x %d bins x 8)", fnd, nrow, bins);
        if ((rc = rounds.size(u.what, ns, fnd * sizeof(uint32_t) + nrow * (B + 1) * sizeof(unsigned long long), needs))) return rc;
        const size_t per = rounds.per;
        HitsCarve hits(c);
        const auto sizes = hits.part<unsigned long long>(nrow, true);
        const auto hists = hits.part<unsigned long long>(per * nrow * B, true);
        const auto overs = hits.part<unsigned long long>(per * nrow, true);
        const auto counters = hits.part<uint32_t>(per * fnd, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact depth: no device memory for the %zu bytes of a round's counters (%zu samples x %zu records x 4 bytes) and the "
                                   "%zu of its histograms; a smaller DD_DEPTH_MB (%zu MiB now) makes smaller rounds",
                        counters.bytes, per, fnd, hists.bytes + overs.bytes, rounds.budget >> 20);
        unsigned long long *size_dev = hits(sizes), *hist_dev = hits(hists), *over_dev = hits(overs);
        uint32_t* count_dev = hits(counters);
        const uint64_t* table_dev = u.table_dev<uint64_t>();
        DD_HIP(hipMemsetAsync(size_dev, 0, sizes.bytes, u.st));
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(u.rec.order(c, k, &set));
        dd::launch_exact_tally(set, nullptr, 0, 0, n, nq, table_dev, size_dev, size_dev + n, u.st);   // (no sample: the universe's row alone)
        DD_HIP(hipGetLastError());
        DD_HIP(hipMemcpyAsync(size_host.data(), size_dev, nrow * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
        rc = rounds.run(u, nbytes, set, hist_dev, hists.bytes + overs.bytes, count_dev, [&](size_t s0, size_t take) -> int {
            dd::launch_exact_depth_tally(set, count_dev, (int)take, n, nq, bins, table_dev, hist_dev, over_dev, u.st);
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(hist_host.data() + s0 * nrow * B, hist_dev, take * nrow * B * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
            DD_HIP(hipMemcpyAsync(over_host.data() + s0 * nrow, over_dev, take * nrow * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
            return DD_OK;
        });
        if (rc) return rc;
    }
    // bin 0: the row's records less those the sample holds; the total from the bins and the clipped records' overflow
    for (size_t s = 0; s < (size_t)ns; ++s)
        for (size_t r = 0; r < nrow; ++r) {
            unsigned long long* h = hist_host.data() + (s * nrow + r) * B;
            unsigned long long held = 0, sum = over_host[s * nrow + r];
            for (size_t d = 1; d < B; ++d) held += h[d], sum += d * h[d];
            h[0] = size_host[r] - held;
            total[s * nrow + r] = sum;
        }
    for (size_t i = 0; i < hist_host.size(); ++i) hist[i] = hist_host[i];
    return u.done(found);
}

int dd_exact_depth(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const uint64_t* all,
                   const uint64_t* none, int nq, int bins, uint64_t* hist, uint64_t* total, uint64_t* found) {
    if (depth_args(c, paths, n, ns, k, all, none, nq, bins, hist, total, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_depth_device(c, p, s, n, ns, k, all, none, nq, bins, hist, total, found);
    });
}

// ------------------------------------------------------------------- samples laid along the genomes of the universe
// dd_exact_cover.hip: depth's rounds with the record of every target position looked up ONCE, in front of the rounds, and a
// kernel per round that gathers the round's counters through that index into window rows.  The shape of the answer is checked
// like dd_exact_paint's: each target's share of off[] against its token count.
// c->hits: index [the targets' token slots] u32 | per round rows [per][off[nt] - off[0]][6] u32 | counters [per][found] u32.
int dd_exact_cover_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, const int32_t* target, int nt,
                          uint64_t window, uint32_t clip, const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (cover_args(c, fasta_dev, n, ns, k, target, nt, window, clip, off, found) || universe_buffers(fasta_dev, nbytes, n, ns)) return DD_EINVAL;
    if (depth_sample_bytes(nbytes, n, ns)) return DD_EINVAL;
    const uint64_t rows = off[nt] - off[0];   // of one sample (each target's own share is checked once the inputs' token counts are known)
    if (rows && !counts) return fail(DD_EINVAL, "null argument");
    SampleRounds rounds;
    UniverseCall u(c, n, ns, k, "exact cover");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    std::vector<unsigned long long> ntok;   // the shape of the answer: every input's ntok
    if ((rc = exact_read_ntok(c, u.in, 0, n, ntok))) return rc;
    // the targets that hold a token, one launch unit each: the entry's own table
    dd::CoverUnit* units = u.table<dd::CoverUnit>((size_t)nt);
    const ExactShape shape{"target", "rows", window, "window"};
    int nunits = 0;
    size_t target_segments = 0, words = 0;
    for (int t = 0; t < nt; ++t) {
        const unsigned long long tokens = ntok[(size_t)target[t]];
        if (exact_check_shape(shape, t, off, target[t], tokens)) return DD_EINVAL;
        if (!tokens) continue;   // (it owns no row)
        const dd::ExactGenome& eg = u.in.etab[(size_t)target[t]];
        const size_t segs = segments_of(tokens);
        dd::CoverUnit& cu = units[nunits++];
        cu.codes = eg.codes, cu.bad = eg.bad, cu.ntok = eg.ntok, cu.index = words, cu.row0 = off[t] - off[0], cu.genome = target[t];
        words += segs * dd::kSegTokens, target_segments = std::max(target_segments, segs);
    }
    if ((rc = u.records(false))) return rc;
    if (u.rec.found >> 31)
        return fail(DD_EINVAL, "exact cover: the universe holds %llu distinct k-mers, a position's index word holds a record below 2^31 (and the "
                               "private flag); lay the samples along a smaller universe",
                    u.rec.found);
    const size_t R = (size_t)rows, row_words = R * dd::kCoverColumns;
    std::vector<uint32_t> host((size_t)ns * row_words, 0u);
    if (u.rec.kept && R) {
        // a round's row: the sample's counters and its windows
        const size_t fnd = (size_t)u.rec.found;
        char needs[160];
        snprintf(needs, sizeof needs, " (%zu records x 4 bytes of counters, and %zu windows x %d columns x 4)", fnd, R, dd::kCoverColumns);
        if ((rc = rounds.size(u.what, ns, fnd * sizeof(uint32_t) + row_words * sizeof(uint32_t), needs))) return rc;
        const size_t per = rounds.per;
        HitsCarve hits(c);
        const auto index = hits.part<uint32_t>(words, true);
        const auto windows = hits.part<uint32_t>(per * row_words, true);
        const auto counters = hits.part<uint32_t>(per * fnd, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact cover: no device memory for the %zu bytes of the targets' index (%zu token slots x 4 bytes), the %zu of a round's "
                                   "counters (%zu samples x %zu records x 4 bytes) and the %zu of its windows; a smaller DD_DEPTH_MB (%zu MiB now) makes "
                                   "smaller rounds",
                        index.bytes, words, counters.bytes, per, fnd, windows.bytes, rounds.budget >> 20);
        uint32_t *index_dev = hits(index), *rows_dev = hits(windows), *count_dev = hits(counters);
        const dd::CoverUnit* units_dev = u.table_dev<dd::CoverUnit>();
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(u.rec.order(c, k, &set));
        dd::launch_exact_cover_index(units_dev, nunits, target_segments, k, c->canonical, set, index_dev, u.st);
        DD_HIP(hipGetLastError());
        rc = rounds.run(u, nbytes, set, rows_dev, windows.bytes, count_dev, [&](size_t s0, size_t take) -> int {
            dd::launch_exact_cover(units_dev, nunits, target_segments, index_dev, count_dev, fnd, (int)take, (size_t)(window / dd::kSegTokens), clip, R,
                                   rows_dev, u.st);
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(host.data() + s0 * row_words, rows_dev, take * row_words * sizeof(uint32_t), hipMemcpyDeviceToHost, u.st));
            return DD_OK;
        });
        if (rc) return rc;
    }
    // sample s owns counts[s][off[0] .. off[nt]-1] of its off[nt] rows
    for (size_t s = 0; s < (size_t)ns && R; ++s)
        memcpy(counts + (s * (size_t)off[nt] + (size_t)off[0]) * dd::kCoverColumns, host.data() + s * row_words, row_words * sizeof(uint32_t));
    return u.done(found);
}

int dd_exact_cover(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, const int32_t* target, int nt,
                   uint64_t window, uint32_t clip, const uint64_t* off, uint32_t* counts, uint64_t* found) {
    if (cover_args(c, paths, n, ns, k, target, nt, window, clip, off, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_cover_device(c, p, s, n, ns, k, target, nt, window, clip, off, counts, found);
    });
}

// ------------------------------------------------------------------- samples explained by the genomes, one by one
// dd_exact_gather.hip: depth's rounds with a walk behind depth_kernel -- per step one pass over the round's counters and the
// masks, one pick per sample -- and one closing pass and pick for the last pick's depth.  The whole walk is enqueued on the
// call's stream; the host sees the round's rows once, behind it.
// c->hits: per round state [per] | step counters [per][64] u64 | sums [per][3] u64 | pick [per][steps] i32 | unique, depth
// [per][steps] u64 | shared [per][n] u64 | counters [per][found] u32.
int dd_exact_gather_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int ns, int k, uint32_t min_hits, int steps,
                           int32_t* pick, uint64_t* unique, uint64_t* depth, uint64_t* shared, uint64_t* total, uint64_t* found) {
    if (gather_args(c, fasta_dev, n, ns, k, min_hits, steps, pick, unique, depth, shared, total, found) || universe_buffers(fasta_dev, nbytes, n, ns))
        return DD_EINVAL;
    if (depth_sample_bytes(nbytes, n, ns)) return DD_EINVAL;
    SampleRounds rounds;
    UniverseCall u(c, n, ns, k, "exact gather");
    int rc;
    if ((rc = u.prepare(fasta_dev, nbytes))) return rc;
    const size_t S = (size_t)steps, N = (size_t)n;
    std::vector<int32_t> pick_host((size_t)ns * S, -1);
    std::vector<unsigned long long> unique_host((size_t)ns * S, 0ull), depth_host((size_t)ns * S, 0ull), shared_host((size_t)ns * N, 0ull),
        sums_host((size_t)ns * dd::kGatherSums, 0ull);
    u.table<uint64_t>(0);   // (no table of its own)
    if ((rc = u.records(false))) return rc;
    if (u.rec.kept) {
        // a round's row: the sample's counters and its walk
        const size_t fnd = (size_t)u.rec.found;
        const size_t walk = sizeof(dd::GatherState) + (64 + dd::kGatherSums + 2 * S + N) * sizeof(unsigned long long) + S * sizeof(int32_t);
        char needs[160];
        snprintf(needs, sizeof needs, " (%zu records x 4 bytes of counters, and %zu of the walk's state and %d steps)", fnd, walk, steps);
        if ((rc = rounds.size(u.what, ns, fnd * sizeof(uint32_t) + walk, needs))) return rc;
        const size_t per = rounds.per;
        HitsCarve hits(c);
        const auto states = hits.part<dd::GatherState>(per, true);
        const auto stepped = hits.part<unsigned long long>(per * 64, true);
        const auto summed = hits.part<unsigned long long>(per * dd::kGatherSums, true);
        const auto picked = hits.part<int32_t>(per * S, true);
        const auto uniques = hits.part<unsigned long long>(per * S, true);
        const auto depths = hits.part<unsigned long long>(per * S, true);
        const auto shareds = hits.part<unsigned long long>(per * N, true);
        const auto counters = hits.part<uint32_t>(per * fnd, false);
        if (hits.reserve())
            return fail(DD_ENOMEM, "exact gather: no device memory for the %zu bytes of a round's counters (%zu samples x %zu records x 4 bytes) and the "
                                   "%zu of its walks; a smaller DD_DEPTH_MB (%zu MiB now) makes smaller rounds",
                        counters.bytes, per, fnd, counters.at, rounds.budget >> 20);
        dd::GatherState* state_dev = hits(states);
        unsigned long long *step_dev = hits(stepped), *sums_dev = hits(summed), *unique_dev = hits(uniques), *depth_dev = hits(depths),
                           *shared_dev = hits(shareds);
        int32_t* pick_dev = hits(picked);
        uint32_t* count_dev = hits(counters);
        Span sp(c, DD_KERNEL_EXACT);
        dd::LocateSet set{};
        DD_HIP(u.rec.order(c, k, &set));
        rc = rounds.run(u, nbytes, set, state_dev, counters.at, count_dev, [&](size_t s0, size_t take) -> int {
            for (int t = 0; t <= steps; ++t) {   // (t == steps: the closing pass, for the last pick's depth)
                dd::launch_exact_gather(set, count_dev, (int)take, n, state_dev, step_dev, sums_dev, u.st);
                dd::launch_exact_gather_pick((int)take, n, t, steps, min_hits, state_dev, step_dev, sums_dev, pick_dev, unique_dev, depth_dev,
                                             shared_dev, u.st);
            }
            DD_HIP(hipGetLastError());
            DD_HIP(hipMemcpyAsync(pick_host.data() + s0 * S, pick_dev, take * S * sizeof(int32_t), hipMemcpyDeviceToHost, u.st));
            DD_HIP(hipMemcpyAsync(unique_host.data() + s0 * S, unique_dev, take * S * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
            DD_HIP(hipMemcpyAsync(depth_host.data() + s0 * S, depth_dev, take * S * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
            DD_HIP(hipMemcpyAsync(shared_host.data() + s0 * N, shared_dev, take * N * sizeof(unsigned long long), hipMemcpyDeviceToHost, u.st));
            DD_HIP(hipMemcpyAsync(sums_host.data() + s0 * dd::kGatherSums, sums_dev, take * dd::kGatherSums * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, u.st));
            return DD_OK;
        });
        if (rc) return rc;
    }
    for (size_t i = 0; i < pick_host.size(); ++i) pick[i] = pick_host[i], unique[i] = unique_host[i], depth[i] = depth_host[i];
    for (size_t i = 0; i < shared_host.size(); ++i) shared[i] = shared_host[i];
    for (size_t s = 0; s < (size_t)ns; ++s)
        total[2 * s] = sums_host[s * dd::kGatherSums + dd::kGatherHeld], total[2 * s + 1] = sums_host[s * dd::kGatherSums + dd::kGatherHeldDepth];
    return u.done(found);
}

int dd_exact_gather(dd_ctx* c, const char* const* paths, int n, const char* const* samples, int ns, int k, uint32_t min_hits, int steps,
                    int32_t* pick, uint64_t* unique, uint64_t* depth, uint64_t* shared, uint64_t* total, uint64_t* found) {
    if (gather_args(c, paths, n, ns, k, min_hits, steps, pick, unique, depth, shared, total, found)) return DD_EINVAL;
    return universe_path_form(c, paths, n, samples, ns, [&](auto p, auto s) {
        return dd_exact_gather_device(c, p, s, n, ns, k, min_hits, steps, pick, unique, depth, shared, total, found);
    });
}

}  // extern "C"
