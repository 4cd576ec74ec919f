// dd_exact_passes.hip -- the host side that every exact entry point stands on (dd_exact_host.h): the call frame and the path
// forms' upload, K0 over the inputs, the pass driver (extract -> the caller's sort and what follows, in one pass or in
// passes over disjoint parts of the k-mer space) and the ordered-record step (the emission of the selected k-mers, its
// sanity check, the room for their order).  No kernels here.
#include "dd_exact_host.h"

// ------------------------------------------------------------------------ the call frame
int exact_args(dd_ctx* c, const void* inputs, int n, int nmax, int kmin, int kmax, const void* out) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || n > nmax)
        return nmax == 16    ? fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n)
               : nmax == 255 ? fail(DD_EINVAL, "n=%d outside 1..255: a membership row has one bit per input, the sort one byte for it", n)
                             : fail(DD_EINVAL, "n=%d outside 1..64: a membership mask has one bit per input", n);
    if (!inputs || !out) return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    return DD_OK;
}

int exact_frame(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int nmax, int kmin, int kmax,
                const void* out, bool more_null) {
    if (exact_args(c, fasta_dev, n, nmax, kmin, kmax, out)) return DD_EINVAL;
    if (!nbytes || more_null) return fail(DD_EINVAL, "null argument");
    return exact_check_inputs(fasta_dev, nbytes, n);
}

int exact_check_inputs(const uint8_t* const* fasta_dev, const size_t* nbytes, int n) {
    for (int g = 0; g < n; ++g) {
        if (nbytes[g] && !fasta_dev[g]) return fail(DD_EINVAL, "input %d: null buffer", g);
        if (reinterpret_cast<uintptr_t>(fasta_dev[g]) & 15)
            return fail(DD_EINVAL, "input %d: device buffer must be 16-byte aligned", g);
    }
    return DD_OK;
}

int exact_check_bits(const char* who, int i, uint64_t all, uint64_t none, int n) {
    const uint64_t outside = n == 64 ? 0ull : ~((1ull << n) - 1ull);
    return (all | none) & outside ? fail(DD_EINVAL, "%s %d: a bit outside 0..%d is set", who, i, n - 1) : DD_OK;
}

int exact_check_shape(const ExactShape& s, int i, const uint64_t* off, int input, unsigned long long ntok) {
    const uint64_t have = off[i + 1] - off[i], want = (ntok + s.unit - 1) / s.unit;
    if (have == want) return DD_OK;
    char holder[32] = "it";
    if (input >= 0) snprintf(holder, sizeof holder, "input %d", input);
    return fail(DD_EINVAL, "%s %d: off[%d] - off[%d] = %llu %s, %llu expected (%s holds %llu tokens, %llu to a %s)", s.who, i, i + 1, i,
                (unsigned long long)have, s.parts, (unsigned long long)want, holder, ntok, (unsigned long long)s.unit, s.unit_name);
}

int select_table(const uint64_t* all, const uint64_t* none, int nq, int n, std::vector<uint64_t>& table) {
    if (!all || !none) return fail(DD_EINVAL, "null argument");
    if (nq < 1) return fail(DD_EINVAL, "nq=%d: at least one query", nq);
    table.resize((size_t)2 * nq);
    for (int q = 0; q < nq; ++q) {
        if (exact_check_bits("query", q, all[q], none[q], n)) return DD_EINVAL;
        table[(size_t)2 * q] = all[q], table[(size_t)2 * q + 1] = none[q];
    }
    return DD_OK;
}

int exact_upload_files(dd_ctx* c, const char* const* paths, int n, const ExactDeviceForm& device_form) {
    DeviceGuard guard(c->device);
    std::vector<size_t> offs(n), sizes(n, 0);
    std::vector<dd::FileBuf> bufs(n);
    std::vector<const uint8_t*> ptrs(n, nullptr);
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        std::string err;
        if (!paths[i] || !dd::read_fasta_file(paths[i], bufs[i], err, usable_cpus())) return fail(DD_EIO, "%s", err.c_str());
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
    bufs.clear();
    return device_form(ptrs.data(), sizes.data());
}

int exact_path_form(dd_ctx* c, const char* const* paths, int n, int nmax, int kmin, int kmax, const void* out, const ExactDeviceForm& device_form) {
    if (exact_args(c, paths, n, nmax, kmin, kmax, out)) return DD_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!paths[i]) return fail(DD_EINVAL, "null argument");
    return exact_upload_files(c, paths, n, device_form);
}

// ------------------------------------------------------------------------ the inputs
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

int exact_read_ntok(dd_ctx* c, const ExactInputs& in, int first, int count, std::vector<unsigned long long>& ntok) {
    ntok.assign((size_t)count, 0ull);
    if (in.etab.empty()) return DD_OK;   // (no input has a token: K0 did not run)
    for (int i = 0; i < count; ++i)
        DD_HIP(hipMemcpyAsync(&ntok[(size_t)i], in.etab[(size_t)(first + i)].ntok, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

size_t exact_budget(const char* env_mb, size_t unset) {
    size_t budget = unset;
    if (const char* e = getenv(env_mb)) budget = (size_t)std::max(1, atoi(e)) << 20;
    return budget;
}

// ------------------------------------------------------------------------ the pass driver
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

// The k-mers of the prepared inputs for one k, extracted into c->exact and handed to consume(arrays, count) -- which
// launches its sort and what follows -- everything at once when that fits exact_budget(), else in passes over disjoint
// parts of the k-mer space.  KMC unions arbitrarily many databases (lib/sketch_classes.py:453-465 of the reference); so
// must this.  The counters are zeroed before each pass, outside its timing span.  `counted` receives them after the
// pass; without it a single pass is not waited for.  c->st_blocks = the number of passes (dd_last_sketch_stats).
int exact_passes(dd_ctx* c, const ExactInputs& in, int n, int k, const ExactLayout& L, const ExactConsume& consume, const ExactCounted& counted) {
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

int exact_sorted_passes(dd_ctx* c, const ExactInputs& in, int n, int k, const char* what, const ExactSortedThen& then,
                        size_t (*scratch_bytes)(size_t keys)) {
    const ExactLayout L{what, dd::exact_tag_mode(k), dd::exact_sched_temp_bytes, scratch_bytes ? scratch_bytes : dd::exact_sched_scratch_bytes};
    return exact_passes(c, in, n, k, L, [&](const ExactArrays& a, size_t count) -> int {
        dd::ExactSorted sorted{};
        DD_HIP(dd::launch_exact_sort_tagged(a.lo, a.hi, a.lo_alt, a.hi_alt, a.g, a.g_alt, count, k, a.temp, a.temp_bytes, c->stream, &sorted));
        DD_HIP(then(sorted, count, a.scratch));
        return DD_OK;
    });
}

// ------------------------------------------------------------------------ the ordered-record step
int exact_records(dd_ctx* c, const ExactInputs& in, int n, int k, const char* what, const ExactSlotsOf* slots, int nq, const void* image,
                  size_t image_bytes, size_t dcap, ExactRecords& r) {
    hipStream_t st = c->stream;
    int rc;
    const size_t stride = align_up(dcap * sizeof(uint64_t), 256), bytes = 256 + 3 * stride;
    if (c->emit.reserve(bytes))
        return slots ? fail(DD_ENOMEM, "%s: no device memory for the %zu bytes of the record area (24 bytes per k-mer slot of the %s)", what, bytes, slots->of)
                     : fail(DD_ENOMEM, "%s: no device memory for an output of %zu records (24 bytes each); ask with a smaller cap", what, dcap);
    char* eb = static_cast<char*>(c->emit.p);
    dd::ExactEmit& e = r.e;
    e = dd::ExactEmit{n, nq, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<unsigned long long*>(eb), dcap};
    if (dcap) {
        e.lo = reinterpret_cast<uint64_t*>(eb + 256);
        e.hi = reinterpret_cast<uint64_t*>(eb + 256 + stride);
        e.mask = reinterpret_cast<uint64_t*>(eb + 256 + 2 * stride);
    }
    DD_HIP(hipMemsetAsync(eb, 0, 256, st));
    if ((rc = stage_table(c, c->ord, image, image_bytes))) return rc;
    e.table = static_cast<const uint64_t*>(c->ord.p);
    rc = exact_sorted_passes(c, in, n, k, what, [&](const dd::ExactSorted& sorted, size_t count, void* scratch) {
        return dd::launch_exact_emit(sorted, count, k, e, scratch, st);
    });
    if (rc) return rc;
    DD_HIP(hipMemcpyAsync(&r.found, e.cursor, sizeof r.found, hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    if (slots && r.found > dcap) return fail(DD_EHIP, "%s: %llu records emitted, the %s %zu k-mer slots", what, r.found, slots->have, dcap);
    r.kept = r.found && r.found <= dcap;
    // (a pass holds an arbitrary part of the k-mer space and its chunks finish in any order: one ordering, after the last)
    const size_t room = r.kept ? dd::exact_emit_order_bytes((size_t)r.found, k) : 0;
    if (c->exact.reserve(room)) return fail(DD_ENOMEM, "%s: no device memory for the %zu bytes that put %llu records in order", what, room, r.found);
    return DD_OK;
}
