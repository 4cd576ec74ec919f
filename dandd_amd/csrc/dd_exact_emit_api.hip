// dd_exact_emit_api.hip -- the exact entry points of the C ABI (include/dandd_hip.h) that hand k-mers out instead of counting
// them.  Two look k-mers up in the ordered records of one emission: the selected k-mers themselves (dd_exact_select_kmers)
// and where they lie in each genome (dd_exact_locate).  Each is its own argument rules, the ordered-record step of
// dd_exact_host.h (exact_records, then ExactRecords::order inside the entry's timing span) and the kernels that read the
// ordered set.  The five entries that look up samples that are no inputs stand on the same step, in dd_exact_samples_api.hip.
// dd_exact_patterns hands out no k-mer but is ragged like the others -- one k per call, a cap and a count -- and
// dd_fasta_index is the record index of a file that turns places into names.
// Host-side orchestration only; the kernels are in dd_exact_sched.hip (emit_kernel, AccPatterns), dd_exact_locate.hip and
// dd_exact_patterns.hip.
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
    const ExactShape shape{"job", "words", (uint64_t)dd::kSegTokens, "word"};
    for (int j = 0; j < njobs; ++j) {
        if (exact_check_shape(shape, j, off, genome[j], ntok[(size_t)genome[j]])) return DD_EINVAL;
        max_segments = std::max(max_segments, (size_t)(off[j + 1] - off[j]));   // (a word per segment)
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
