// dd_api.hip -- the C ABI of libdandd_hip.so (declared in include/dandd_hip.h).
//
// Host-side orchestration only: workspace management in HBM, job tables for the sweep,
// stream/event plumbing.  Every entry point names the DandD command line it replaces in
// include/dandd_hip.h.  There is no CPU fallback anywhere in this file.  The file-ingestion
// pipeline (dd_sketch_fasta, dd_sketch_files, dd_inflate_files) is in dd_ingest.hip.
#include <memory>
#include <mutex>
#include "dd_ctx.h"

using dd::FileBuf;
using dd::read_fasta_file;

thread_local std::string g_err;   // (declared in dd_ctx.h)

namespace {

hipEvent_t get_event(dd_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct Span {  // brackets a launch (or a whole phase) on the context's stream with events when timing is on
    dd_ctx* c;
    int which;
    bool on;
    TimedSpan s{};
    Span(dd_ctx* c_, int which_, bool on_ = true) : c(c_), which(which_), on(on_ && c_->timing) {
        if (on) {
            s.a = get_event(c);
            s.b = get_event(c);
            (void)hipEventRecord(s.a, c->stream);
        }
    }
    ~Span() {
        if (on) {
            (void)hipEventRecord(s.b, c->stream);
            c->spans[which].push_back(s);
        }
    }
};

// upload a host table through the pinned staging buffer (async on the stream)
int upload(dd_ctx* c, HostBuf& stage, void* dst_dev, const void* src, size_t bytes, size_t stage_off) {
    if (!bytes) return DD_OK;
    memcpy(static_cast<char*>(stage.p) + stage_off, src, bytes);
    DD_HIP(hipMemcpyAsync(dst_dev, static_cast<char*>(stage.p) + stage_off, bytes,
                          hipMemcpyHostToDevice, c->stream));
    return DD_OK;
}


// histograms already on the device -> estimates on the host (device MLE, bit-identical to the
// host MLE: same IEEE operations, no contraction; asserted by tests/test_gpu_parity.py)
int estimates_from_hist(dd_ctx* c, const uint32_t* hist_dev, size_t njobs, double* est_host) {
    int rc = c->est.reserve(njobs * sizeof(double));
    if (rc) return rc;
    dd::launch_mle(hist_dev, njobs, c->p, static_cast<double*>(c->est.p), c->stream);
    DD_HIP(hipGetLastError());
    DD_HIP(hipMemcpyAsync(est_host, c->est.p, njobs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

}  // namespace

extern "C" {

int dd_abi_version(void) { return DD_ABI_VERSION; }

const char* dd_last_error(void) { return g_err.c_str(); }

dd_ctx* dd_create(int device, int log2m, int canonical) {
    if (log2m < 4 || log2m > 20) {
        fail(DD_EINVAL, "log2m=%d outside 4..20", log2m);
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        fail(DD_ENODEV, "no HIP device visible (%s): libdandd_hip has no CPU path",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(DD_ENODEV, "device %d not in 0..%d", device, ndev - 1);
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        fail(DD_ENODEV, "hipGetDeviceProperties(%d) failed", device);
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(DD_ENODEV, "device %d is %s; this library is built for gfx950 only", device,
             prop.gcnArchName);
        return nullptr;
    }
    dd_ctx* c = new dd_ctx();
    c->device = device;
    c->p = log2m;
    c->canonical = canonical ? 1 : 0;
    c->bucket_budget = std::min<size_t>((size_t)48 << 30, std::max<size_t>((size_t)16 << 30, prop.totalGlobalMem / 6));
    DeviceGuard g(device);
    if (hipEventCreateWithFlags(&c->stage_free, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->stage_free_alt, hipEventDisableTiming) != hipSuccess) {
        fail(DD_ENODEV, "hipEventCreate failed");
        delete c;
        return nullptr;
    }
    return c;
}

void dd_destroy(dd_ctx* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)dd_comm_destroy(c);
    for (auto& v : c->spans)
        for (auto& s : v) {
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->stage_free) (void)hipEventDestroy(c->stage_free);
    if (c->stage_free_alt) (void)hipEventDestroy(c->stage_free_alt);
    for (auto& pe : c->plans) pe.jobtab.release();
    for (DevBuf* b : {&c->tokens, &c->scratch, &c->tables, &c->fasta, &c->regs, &c->ptrs, &c->hist,
                      &c->est, &c->ord, &c->bitmaps, &c->bigmaps, &c->exact, &c->buckets, &c->gram, &c->synth})
        b->release();
    for (HostBuf* b : {&c->stage, &c->stage_jobs, &c->stage_rows, &c->stage_alt, &c->stage_jobs_alt, &c->stage_rows_alt}) b->release();
    c->ingest.release();
    for (int i = 0; i < 8; ++i)
        if (c->side[i]) {
            (void)hipStreamDestroy(c->side[i]);
            (void)hipEventDestroy(c->side_done[i]);
        }
    if (c->side_go) {
        (void)hipEventDestroy(c->side_go);
    }
    delete c;
}

int dd_set_stream(dd_ctx* c, void* hip_stream) {
    if (check_ctx(c)) return DD_EINVAL;
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next != c->stream) {
        // Work queued on the old stream still uses the context's tables and workspaces (the cached K1 job
        // tables were uploaded there); nothing orders a new stream behind it, so it is drained first.
        DeviceGuard g(c->device);
        // The old handle is not touched: a caller may hand over a new stream because it already destroyed the old
        // one, and synchronising a destroyed hipStream_t is undefined.  Draining the device covers the old stream
        // whether it still exists or not (destroying a stream lets its queued work finish); switching streams is rare.
        DD_HIP(hipDeviceSynchronize());
        c->stream = next;
    }
    return DD_OK;
}

int dd_synchronize(dd_ctx* c) {
    if (check_ctx(c)) return DD_EINVAL;
    DeviceGuard g(c->device);
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// ------------------------------------------------------------------------------ sketch
// The side streams the k classes of a call run on: `n` of them (at most 8), made when first asked for -- a stream
// costs 2 ms to create and as much again to destroy, which a one-shot process pays in full.
static int ensure_side_streams(dd_ctx* c, int n) {
    if (!c->side_go) DD_HIP(hipEventCreateWithFlags(&c->side_go, hipEventDisableTiming));
    for (int i = 0; i < std::min(n, 8); ++i) {
        if (c->side[i]) continue;
        DD_HIP(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        DD_HIP(hipEventCreateWithFlags(&c->side_done[i], hipEventDisableTiming));
    }
    return DD_OK;
}

int dd_sketch_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int ngenomes,
                     int kmin, int kmax, uint8_t* regs_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (ngenomes < 0 || !regs_dev || (ngenomes && (!fasta_dev || !nbytes)))
        return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    for (int g = 0; g < ngenomes; ++g) {
        if (nbytes[g] && !fasta_dev[g]) return fail(DD_EINVAL, "genome %d: null buffer", g);
        if (reinterpret_cast<uintptr_t>(fasta_dev[g]) & 15)
            return fail(DD_EINVAL, "genome %d: device buffer must be 16-byte aligned", g);
    }
    DeviceGuard guard(c->device);
    const int p = c->p, K = kmax - kmin + 1;
    const size_t m = (size_t)1 << p;
    hipStream_t st = c->stream;

    DD_HIP(hipMemsetAsync(regs_dev, 0, (size_t)ngenomes * K * m, st));
    if (!ngenomes) return DD_OK;

    // ---- workspace: token streams of all genomes + one K0 scratch --------------------
    std::vector<size_t> off_codes(ngenomes), off_bad(ngenomes), off_ntok(ngenomes);
    size_t tot = 0, max_n = 0;
    for (int g = 0; g < ngenomes; ++g) {
        off_codes[g] = tot;
        tot += align_up(dd::codes_words(nbytes[g]) * 4, 256);
        off_bad[g] = tot;
        tot += align_up(dd::bad_words(nbytes[g]) * 4, 256);
        off_ntok[g] = tot;
        tot += 256;
        max_n = std::max(max_n, nbytes[g]);
    }
    std::vector<size_t> off_scratch(ngenomes);
    size_t scratch_tot = 0;
    for (int g = 0; g < ngenomes; ++g) {
        off_scratch[g] = scratch_tot;
        scratch_tot += align_up(dd::pack_scratch_bytes(nbytes[g]), 256);
    }
    int rc;
    if ((rc = c->tokens.reserve(tot))) return rc;
    if ((rc = c->scratch.reserve(scratch_tot))) return rc;
    char* tb = static_cast<char*>(c->tokens.p);
    char* sb = static_cast<char*>(c->scratch.p);

    // presence bitmaps for the small-k class (k <= 9), zeroed per call
    const bool use_bitmaps = kmin <= dd::kBitmapMaxK;
    uint32_t* bitmap_base = nullptr;
    if (use_bitmaps) {
        const size_t bbytes = (size_t)ngenomes * dd::kBitmapStride * sizeof(uint32_t);
        if ((rc = c->bitmaps.reserve(bbytes))) return rc;
        bitmap_base = static_cast<uint32_t*>(c->bitmaps.p);
        DD_HIP(hipMemsetAsync(bitmap_base, 0, bbytes, st));
    }

    // ... and for k = 10 (, 11) at log2m >= 19 (dd_kernels.h)
    uint32_t* bigmap_base = nullptr;
    size_t bigmap_stride = 0;
    {
        int ka = 0, kb = 0;
        if (dd::plan_bigmap_range(p, kmin, kmax, dd::PlanKnobs::from_env(), nbytes, ngenomes, &ka, &kb)) {
            bigmap_stride = dd::bigmap_offset_words(kb + 1, c->canonical != 0);
            const size_t bbytes = (size_t)ngenomes * bigmap_stride * sizeof(uint32_t);
            if ((rc = c->bigmaps.reserve(bbytes))) return rc;
            bigmap_base = static_cast<uint32_t*>(c->bigmaps.p);
            DD_HIP(hipMemsetAsync(bigmap_base, 0, bbytes, st));
        }
    }

    // ---- K0 / K1 genome tables -----------------------------------------------------------
    std::vector<dd::SweepGenome> gtab(ngenomes);
    std::vector<dd::PackGenome> ptab(ngenomes);
    uint64_t tokens_ub = 0;
    size_t max_chunks = 0;
    for (int g = 0; g < ngenomes; ++g) {
        dd::TokenStream ts{reinterpret_cast<uint32_t*>(tb + off_codes[g]),
                           reinterpret_cast<uint32_t*>(tb + off_bad[g]),
                           reinterpret_cast<unsigned long long*>(tb + off_ntok[g])};
        ptab[g] = dd::PackGenome{fasta_dev[g], nbytes[g], dd::pack_chunks(nbytes[g]),
                                 reinterpret_cast<long long*>(sb + off_scratch[g]), ts};
        max_chunks = std::max(max_chunks, ptab[g].nchunks);
        gtab[g] = dd::SweepGenome{ts.codes, ts.bad, ts.ntok, regs_dev + (size_t)g * K * m,
                                  bitmap_base ? bitmap_base + (size_t)g * dd::kBitmapStride : nullptr,
                                  bigmap_base ? bigmap_base + (size_t)g * bigmap_stride : nullptr};
        tokens_ub += nbytes[g];
    }
    (void)max_n;

    // ---- genome tables up, K0 launched: the K1 job tables are planned on the host meanwhile -------
    const size_t pack_off = align_up(sizeof(dd::SweepGenome) * ngenomes, 256);
    const size_t gtab_bytes = pack_off + align_up(sizeof(dd::PackGenome) * ngenomes, 256);
    if ((rc = c->tables.reserve(gtab_bytes))) return rc;
    // the staging buffers may still be feeding the uploads of the call before last (they alternate: dd_ctx)
    std::swap(c->stage, c->stage_alt);
    std::swap(c->stage_jobs, c->stage_jobs_alt);
    std::swap(c->stage_rows, c->stage_rows_alt);
    std::swap(c->stage_free, c->stage_free_alt);
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(gtab_bytes))) return rc;
    char* tdev = static_cast<char*>(c->tables.p);
    if ((rc = upload(c, c->stage, tdev, gtab.data(), sizeof(dd::SweepGenome) * ngenomes, 0))) return rc;
    if ((rc = upload(c, c->stage, tdev + pack_off, ptab.data(), sizeof(dd::PackGenome) * ngenomes, pack_off))) return rc;
    {
        Span sp(c, DD_KERNEL_PACK);  // K0: pack every genome of the batch (three launches)
        dd::launch_pack_batch(reinterpret_cast<const dd::PackGenome*>(tdev + pack_off), ngenomes,
                              max_chunks, st);
    }
    DD_HIP(hipGetLastError());

    // ---- K1 job tables (dd_plan.hip), built while K0 runs -----------------------------------
    dd::PlanKnobs knobs = dd::PlanKnobs::from_env();
    // (longer epochs = fewer launches and sharper filters per record: +4 % on 13 x 3 Gbp at log2m 20 with 48 GiB)
    if (!getenv("DD_BUCKET_GB")) knobs.bucket_budget = c->bucket_budget;
    dd_ctx::PlanEntry* hit = nullptr;
    dd_ctx::PlanEntry* oldest = &c->plans[0];
    for (auto& pe : c->plans) {
        if (pe.valid && pe.kmin == kmin && pe.kmax == kmax && pe.knobs == knobs && pe.sizes.size() == (size_t)ngenomes &&
            std::equal(pe.sizes.begin(), pe.sizes.end(), nbytes))
            hit = &pe;
        if (pe.last_use < oldest->last_use) oldest = &pe;
    }
    auto& pc = hit ? *hit : *oldest;
    pc.last_use = ++c->plan_clock;
    if (!hit) {
        // (the entry being replaced may still be read by kernels of an earlier call: its device table is only ever
        // written by copies on this same stream, and a table that must grow is freed by hipFree, which waits)
        pc.valid = false;
        pc.classes = dd::plan_sweep(p, c->canonical, nbytes, ngenomes, kmin, kmax, knobs);
        size_t job_bytes = 0;
        pc.job_off.assign(pc.classes.size(), 0);
        for (size_t i = 0; i < pc.classes.size(); ++i) {
            pc.job_off[i] = job_bytes;
            job_bytes += align_up(sizeof(dd::SweepJob) * pc.classes[i].jobs.size(), 256);
        }
        if ((rc = pc.jobtab.reserve(job_bytes))) return rc;
        if ((rc = c->stage_jobs.reserve(job_bytes))) return rc;
        for (size_t i = 0; i < pc.classes.size(); ++i)
            if ((rc = upload(c, c->stage_jobs, static_cast<char*>(pc.jobtab.p) + pc.job_off[i], pc.classes[i].jobs.data(),
                             sizeof(dd::SweepJob) * pc.classes[i].jobs.size(), pc.job_off[i])))
                return rc;
        pc.kmin = kmin;
        pc.kmax = kmax;
        pc.knobs = knobs;
        pc.sizes.assign(nbytes, nbytes + ngenomes);
        pc.valid = true;
    }
    const std::vector<dd::SweepClass>& classes = pc.classes;
    const std::vector<size_t>& job_off = pc.job_off;
    char* jdev = static_cast<char*>(pc.jobtab.p);
    DD_HIP(hipEventRecord(c->stage_free, st));

    // ---- bucket mode (log2m >= 17): row table, cursors, filters and record areas ----------------
    const dd::SweepPlan* bplan = nullptr;
    for (const dd::SweepClass& sc : classes)
        if (sc.plan.mode == dd::kBucketMode) bplan = &sc.plan;
    const dd::BucketRow* rows_dev = nullptr;
    const int nrows = ngenomes * K;
    if (bplan) {
        const size_t flt_bytes = align_up((m >> bplan->logg) / 2, 16), area_bytes = (size_t)bplan->cap_chunks * 4096;  // 4-bit filter entries; 1024 records per chunk
        const size_t fill_bytes = align_up((size_t)bplan->cap_chunks * 4, 256) + align_up((size_t)bplan->cap_chunks * 32, 256);  // fill + seg
        int first_hashed = K, hashed_per_genome = 0;  // rows of a genome that belong to a bucket class
        for (const dd::SweepClass& sc : classes)
            if (sc.plan.mode == dd::kBucketMode) {
                first_hashed = std::min(first_hashed, sc.kfirst - kmin);
                hashed_per_genome += sc.klast - sc.kfirst + 1;
            }
        const size_t nhashed = (size_t)ngenomes * hashed_per_genome;
        const size_t tab_bytes = align_up(sizeof(dd::BucketRow) * nrows, 256);
        // one cursor per row, each in a 256-byte slot of its own: every block of a row is reserved by an atomic add on it,
        // and neighbouring rows are written from other XCDs
        const size_t cur_stride = 256;
        const size_t cur_bytes = align_up((size_t)nrows * cur_stride, 256);
        const size_t flt_tot = align_up(nhashed * flt_bytes, 256);
        // the first epoch's updates of rho = 1: one bit per register instead of a record each (dd_sweep.hip,
        // scatter_first_bin_kernel); the bits start at zero with the cursors and filters
        const size_t ones_bytes = m / 8, ones_tot = align_up(nhashed * ones_bytes, 256);
        if ((rc = c->buckets.reserve(tab_bytes + cur_bytes + flt_tot + ones_tot + nhashed * (fill_bytes + area_bytes)))) return rc;
        if ((rc = c->stage_rows.reserve(tab_bytes))) return rc;
        char* bb = static_cast<char*>(c->buckets.p);
        char* fills = bb + tab_bytes + cur_bytes + flt_tot + ones_tot;
        char* areas = fills + nhashed * fill_bytes;
        std::vector<dd::BucketRow> rtab(nrows);
        size_t h = 0;
        for (int g = 0; g < ngenomes; ++g)
            for (int kk = 0; kk < K; ++kk) {
                dd::BucketRow& r = rtab[(size_t)g * K + kk];
                r.regs = regs_dev + ((size_t)g * K + kk) * m;
                r.cursor = reinterpret_cast<uint32_t*>(bb + tab_bytes + ((size_t)g * K + kk) * cur_stride);
                const bool hashed = kk >= first_hashed && kk < first_hashed + hashed_per_genome;
                r.filter = hashed ? reinterpret_cast<uint8_t*>(bb + tab_bytes + cur_bytes + h * flt_bytes) : nullptr;
                r.ones = hashed ? reinterpret_cast<uint32_t*>(bb + tab_bytes + cur_bytes + flt_tot + h * ones_bytes) : nullptr;
                r.fill = hashed ? reinterpret_cast<uint32_t*>(fills + h * fill_bytes) : nullptr;
                r.seg = hashed ? reinterpret_cast<uint16_t*>(fills + h * fill_bytes + align_up((size_t)bplan->cap_chunks * 4, 256)) : nullptr;
                r.area = hashed ? reinterpret_cast<uint32_t*>(areas + h * area_bytes) : nullptr;
                h += hashed ? 1 : 0;
            }
        // cursors, filters and bits start at zero: nothing handed out, every register's lower bound is 0
        DD_HIP(hipMemsetAsync(bb + tab_bytes, 0, cur_bytes + flt_tot + ones_tot, st));
        if ((rc = upload(c, c->stage_rows, bb, rtab.data(), sizeof(dd::BucketRow) * nrows, 0))) return rc;
        rows_dev = reinterpret_cast<const dd::BucketRow*>(bb);
        DD_HIP(hipEventRecord(c->stage_free, st));
    }

    // ---- K1 launches -------------------------------------------------------------------
    auto launch_lds_class = [&](const dd::SweepClass& sc, size_t i, hipStream_t ks) {
        const dd::SweepGenome* gt = reinterpret_cast<const dd::SweepGenome*>(tdev);
        const dd::SweepJob* jt = reinterpret_cast<const dd::SweepJob*>(jdev + job_off[i]);
        if (sc.kclass == dd::kBitmapClass) {
            dd::launch_bitmap(gt, jt, (int)sc.jobs.size(), sc.kfirst, sc.klast, c->canonical, ks);
            dd::launch_bitmap_finish(gt, ngenomes, sc.kfirst, sc.klast, kmin, p, ks);
        } else if (sc.kclass == dd::kBigmapClass) {
            dd::launch_bigmap(gt, jt, (int)sc.jobs.size(), c->canonical, ks);
            dd::launch_bigmap_finish(gt, ngenomes, sc.kfirst, sc.klast, kmin, p, c->canonical, ks);
        } else {
            dd::launch_sweep(gt, jt, (int)sc.jobs.size(), sc.kclass, sc.plan, ks);
        }
    };
    // The k classes are independent.  On a big call they are launched back to back (running them side by side
    // was measured neutral to slightly slower: they compete for the same VALUs).  On a SMALL call -- one batch of
    // the ingestion pipeline, a single genome -- every class is only a few rounds of workgroups long and ends
    // with a tail of idle CUs: there the classes go to side streams so that one's tail overlaps another's body.
    int blocks = 0;
    size_t lds_jobs = 0;
    int lds_classes = 0;
    for (const dd::SweepClass& sc : classes)
        if (sc.plan.mode != dd::kBucketMode) lds_jobs += sc.jobs.size(), ++lds_classes;
    const bool side = lds_classes > 1 && lds_jobs < 12000;
    if (side && (rc = ensure_side_streams(c, lds_classes))) return rc;
    // log2m >= 17, see below.  A call whose only epoch is the unfiltered first one (many small genomes: 64 x 5 Mbp at
    // log2m 20) runs its classes one after the other instead: its scatter (returning LDS atomics, 4-byte stores) and
    // its replay (HBM reads at 5 TB/s) each have the chip to themselves then -- 24.4 -> 22.9 ms with round 4's kernels
    // (profiles/r04_bucket_path.txt); calls with filtered epochs keep the side streams (26.8 against 24.9 ms without).
    const bool side_b = bplan && bplan->nepochs > 1;
    // (launches that run side by side are timed as ONE span on the caller's stream: per-launch spans would overlap)
    std::unique_ptr<Span> phase((side || side_b) ? new Span(c, DD_KERNEL_SWEEP) : nullptr);
    if (side) DD_HIP(hipEventRecord(c->side_go, st));
    int lane_no = 0;
    for (size_t i = 0; i < classes.size(); ++i) {
        const dd::SweepClass& sc = classes[i];
        if (sc.plan.mode == dd::kBucketMode || side_b) continue;
        hipStream_t ks = st;
        if (side) {
            ks = c->side[lane_no & 7];
            DD_HIP(hipStreamWaitEvent(ks, c->side_go, 0));
        }
        Span sp(c, DD_KERNEL_SWEEP, !side);
        launch_lds_class(sc, i, ks);
        if (side) {
            DD_HIP(hipEventRecord(c->side_done[lane_no & 7], ks));
            DD_HIP(hipStreamWaitEvent(st, c->side_done[lane_no & 7], 0));
            ++lane_no;
        }
        blocks += (int)sc.jobs.size();
    }
    if (bplan) {
        // Every k class is a pipeline of its own -- scatter(e), (sort(e),) replay(e), scatter(e+1) ... over its own rows --
        // so, when there are filtered epochs, each gets a side stream: the tails of one class's launches are filled by the
        // others' work.  (Starting the pipelines one first-epoch scatter apart, and streams of different priorities, were
        // measured and lost: profiles/r03_bucket_path.txt, r04_bucket_path.txt.)
        const dd::ScatterParams sp{rows_dev, K, bplan->logg, bplan->cap_chunks, bplan->nb_log2};
        if (side_b && (rc = ensure_side_streams(c, (int)classes.size()))) return rc;
        if (side_b) DD_HIP(hipEventRecord(c->side_go, st));
        int lane_b = 0;
        for (size_t i = 0; i < classes.size(); ++i) {
            const dd::SweepClass& sc = classes[i];
            hipStream_t ks = st;
            if (side_b) {
                ks = c->side[lane_b & 7];
                DD_HIP(hipStreamWaitEvent(ks, c->side_go, 0));
            }
            if (sc.plan.mode != dd::kBucketMode) {
                if (!side_b) continue;  // (already launched above)
                launch_lds_class(sc, i, ks);   // the small-k classes (their rows are not bucketed) run beside the pipelines
                blocks += (int)sc.jobs.size();
            }
            for (int e = 0; sc.plan.mode == dd::kBucketMode && e < bplan->nepochs; ++e) {
                const size_t j0 = sc.epoch_begin[e], j1 = sc.epoch_begin[e + 1];
                if (j1 == j0) continue;
                Span span(c, DD_KERNEL_SWEEP, !side_b);
                dd::launch_scatter(reinterpret_cast<const dd::SweepGenome*>(tdev),
                                   reinterpret_cast<const dd::SweepJob*>(jdev + job_off[i]) + j0, (int)(j1 - j0),
                                   sc.kclass, sc.plan, sp, ks, e == 0);
                dd::launch_replay(rows_dev, ngenomes, K, sc.kfirst - kmin, sc.klast - sc.kfirst + 1, *bplan, ks, e == 0);
                blocks += (int)(j1 - j0);
            }
            if (side_b) {
                DD_HIP(hipEventRecord(c->side_done[lane_b & 7], ks));
                DD_HIP(hipStreamWaitEvent(st, c->side_done[lane_b & 7], 0));
                ++lane_b;
            }
        }
    }
    phase.reset();  // (closes the span: every side stream has been joined into the caller's stream above)
    DD_HIP(hipGetLastError());
    c->st_tokens = tokens_ub;
    c->st_updates = tokens_ub * (uint64_t)K;
    c->st_blocks = blocks;
    return DD_OK;
}

int dd_sketch_buffer(dd_ctx* c, const uint8_t* fasta, size_t nbytes, int kmin, int kmax, uint8_t* regs) {
    if (check_ctx(c)) return DD_EINVAL;
    if (!regs || (nbytes && !fasta)) return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    DeviceGuard guard(c->device);
    const size_t K = (size_t)(kmax - kmin + 1), m = (size_t)1 << c->p;
    int rc;
    // (FASTQ in a host buffer: resolved into the FASTA K0 reads, as the file paths do -- dd_io.h)
    FileBuf fq;
    if (dd::has_plus_line(fasta, nbytes)) {
        if (!fq.reserve(nbytes + 16)) return fail(DD_ENOMEM, "out of host memory");
        fq.len = nbytes = dd::fastq_to_fasta(fasta, nbytes, fq.p);
        fasta = fq.p;
    }
    if ((rc = c->fasta.reserve(nbytes + 16))) return rc;
    if ((rc = c->regs.reserve(K * m))) return rc;
    if (nbytes) DD_HIP(hipMemcpyAsync(c->fasta.p, fasta, nbytes, hipMemcpyHostToDevice, c->stream));
    const uint8_t* ptrs[1] = {static_cast<const uint8_t*>(c->fasta.p)};
    const size_t ns[1] = {nbytes};
    if ((rc = dd_sketch_device(c, ptrs, ns, 1, kmin, kmax, static_cast<uint8_t*>(c->regs.p)))) return rc;
    DD_HIP(hipMemcpyAsync(regs, c->regs.p, K * m, hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// ------------------------------------------------------------------------- exact count
namespace {

// K0 over the n inputs of an exact call (once per call, whatever the number of ks) and where each genome's k-mers go
struct ExactInputs {
    const dd::ExactGenome* etab_dev = nullptr;
    size_t slots = 0, max_segments = 0;   // slots = 0: no input has a token
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
    hipStream_t st = c->stream;
    int rc;
    // token streams (K0), laid out like dd_sketch_device does
    std::vector<size_t> off_codes(n), off_bad(n), off_ntok(n), off_scratch(n);
    size_t tot = 0, scratch_tot = 0, slots = 0, max_segments = 0, max_chunks = 0;
    std::vector<unsigned long long> base(n);
    for (int g = 0; g < n; ++g) {
        off_codes[g] = tot;
        tot += align_up(dd::codes_words(nbytes[g]) * 4, 256);
        off_bad[g] = tot;
        tot += align_up(dd::bad_words(nbytes[g]) * 4, 256);
        off_ntok[g] = tot;
        tot += 256;
        off_scratch[g] = scratch_tot;
        scratch_tot += align_up(dd::pack_scratch_bytes(nbytes[g]), 256);
        base[g] = slots;
        const size_t segs = (nbytes[g] + dd::kSegTokens - 1) / dd::kSegTokens;
        slots += segs * dd::kSegTokens;
        max_segments = std::max(max_segments, segs);
        max_chunks = std::max(max_chunks, dd::pack_chunks(nbytes[g]));
    }
    in.slots = slots, in.max_segments = max_segments;
    if (!slots) return DD_OK;
    if ((rc = c->tokens.reserve(tot))) return rc;
    if ((rc = c->scratch.reserve(scratch_tot))) return rc;
    char* tb = static_cast<char*>(c->tokens.p);
    char* sb = static_cast<char*>(c->scratch.p);

    std::vector<dd::PackGenome> ptab(n);
    std::vector<dd::ExactGenome> etab(n);
    for (int g = 0; g < n; ++g) {
        dd::TokenStream ts{reinterpret_cast<uint32_t*>(tb + off_codes[g]), reinterpret_cast<uint32_t*>(tb + off_bad[g]),
                           reinterpret_cast<unsigned long long*>(tb + off_ntok[g])};
        ptab[g] = dd::PackGenome{fasta_dev[g], nbytes[g], dd::pack_chunks(nbytes[g]),
                                 reinterpret_cast<long long*>(sb + off_scratch[g]), ts};
        etab[g] = dd::ExactGenome{ts.codes, ts.bad, ts.ntok, base[g]};
    }
    const size_t pbytes = align_up(sizeof(dd::PackGenome) * n, 256), ebytes = align_up(sizeof(dd::ExactGenome) * n, 256);
    if ((rc = c->tables.reserve(pbytes + ebytes))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(pbytes + ebytes))) return rc;
    char* tdev = static_cast<char*>(c->tables.p);
    if ((rc = upload(c, c->stage, tdev, ptab.data(), sizeof(dd::PackGenome) * n, 0))) return rc;
    if ((rc = upload(c, c->stage, tdev + pbytes, etab.data(), sizeof(dd::ExactGenome) * n, pbytes))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, st));
    {
        Span sp(c, DD_KERNEL_PACK);
        dd::launch_pack_batch(reinterpret_cast<const dd::PackGenome*>(tdev), n, max_chunks, st);
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

}  // namespace

int dd_exact_count_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int k,
                          uint64_t* distinct) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 0 || !distinct || (n && (!fasta_dev || !nbytes))) return fail(DD_EINVAL, "null argument");
    if (k < 1 || k > 64) return fail(DD_EINVAL, "k=%d outside 1..64", k);
    if (exact_check_inputs(fasta_dev, nbytes, n)) return DD_EINVAL;
    *distinct = 0;
    if (!n) return DD_OK;
    DeviceGuard guard(c->device);
    hipStream_t st = c->stream;
    int rc;
    ExactInputs in;
    if ((rc = exact_prepare(c, fasta_dev, nbytes, n, in))) return rc;
    const size_t slots = in.slots, max_segments = in.max_segments;
    if (!slots) return DD_OK;
    const dd::ExactGenome* etab_dev = in.etab_dev;
    const bool wide = k > 32;
    const size_t arrays = wide ? 4 : 2;
    // HBM for the k-mer arrays (keys + the sort's other half): everything at once when that fits the budget,
    // else in passes over disjoint parts of the k-mer space (below).  KMC unions arbitrarily many databases
    // (/root/reference/lib/sketch_classes.py:453-465); so must this.
    const size_t budget = exact_budget();
    const bool single = arrays * slots * sizeof(uint64_t) <= budget;
    const size_t cap = single ? slots : std::max<size_t>(budget / (arrays * sizeof(uint64_t)), 4096);  // k-mers per pass

    // layout of the k-mer workspace for `cap` keys: counters (256 B) | histogram (32 KiB) | lo | lo_alt [| hi | hi_alt] | temp
    const size_t hist_bytes = (size_t)dd::kExactBins * sizeof(unsigned long long);
    auto carve = [&](size_t keys, size_t temp_bytes, unsigned long long*& counters, unsigned long long*& hist, uint64_t*& lo,
                     uint64_t*& lo_alt, uint64_t*& hi, uint64_t*& hi_alt, void*& temp) -> int {
        const size_t stride = align_up(keys * sizeof(uint64_t), 256);
        int r = c->exact.reserve(256 + hist_bytes + arrays * stride + temp_bytes + 256);
        if (r) return r;
        char* eb = static_cast<char*>(c->exact.p);
        counters = reinterpret_cast<unsigned long long*>(eb);
        hist = reinterpret_cast<unsigned long long*>(eb + 256);
        char* kb = eb + 256 + hist_bytes;
        lo = reinterpret_cast<uint64_t*>(kb);
        lo_alt = reinterpret_cast<uint64_t*>(kb + stride);
        hi = wide ? reinterpret_cast<uint64_t*>(kb + 2 * stride) : nullptr;
        hi_alt = wide ? reinterpret_cast<uint64_t*>(kb + 3 * stride) : nullptr;
        temp = kb + arrays * stride;
        return DD_OK;
    };
    unsigned long long *counters = nullptr, *hist = nullptr;
    uint64_t *lo = nullptr, *lo_alt = nullptr, *hi = nullptr, *hi_alt = nullptr;
    void* temp = nullptr;

    if (single) {
        const size_t key_bytes = slots * sizeof(uint64_t);
        const size_t temp_bytes = dd::exact_sort_temp_bytes(slots, k);
        if ((rc = carve(slots, temp_bytes, counters, hist, lo, lo_alt, hi, hi_alt, temp))) return rc;
        DD_HIP(hipMemsetAsync(counters, 0, 256, st));
        {
            Span sp(c, DD_KERNEL_EXACT);
            DD_HIP(hipMemsetAsync(lo, 0xFF, key_bytes, st));  // unwritten slots read as the all-ones sentinel
            if (wide) DD_HIP(hipMemsetAsync(hi, 0xFF, key_bytes, st));
            dd::launch_kmer_extract(etab_dev, n, max_segments, k, c->canonical, lo, hi, counters, st);
            DD_HIP(hipGetLastError());
            DD_HIP(dd::launch_exact_sort_count(lo, hi, lo_alt, hi_alt, slots, k, temp, temp_bytes, counters, st));
        }
        unsigned long long h[3] = {0, 0, 0};
        DD_HIP(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        // the all-ones group holds the sentinels of unwritten slots and/or genuine T^k k-mers
        const bool sentinel_present = h[0] < (unsigned long long)slots, all_t = h[1] != 0;
        *distinct = h[2] - ((sentinel_present || all_t) ? 1 : 0) + (all_t ? 1 : 0);
        return DD_OK;
    }

    // ---- more k-mers than the budget holds: passes over disjoint parts of the k-mer space ------------
    // The k-mer space is cut into 4096 bins by a mix of the k-mer itself (equal k-mers share a bin), a
    // counting pass sizes the bins, consecutive bins are grouped into passes of at most `cap` k-mers, and every
    // pass extracts (densely), sorts and counts only its own bins: distinct = sum over passes.
    size_t temp_bytes = dd::exact_sort_temp_bytes(cap, k);
    if ((rc = carve(cap, temp_bytes, counters, hist, lo, lo_alt, hi, hi_alt, temp))) return rc;
    DD_HIP(hipMemsetAsync(counters, 0, 256 + hist_bytes, st));
    {
        Span sp(c, DD_KERNEL_EXACT);
        dd::launch_kmer_extract(etab_dev, n, max_segments, k, c->canonical, lo, hi, counters, st, 1, hist, 0, 0);
    }
    DD_HIP(hipGetLastError());
    std::vector<unsigned long long> bins(dd::kExactBins);
    DD_HIP(hipMemcpyAsync(bins.data(), hist, hist_bytes, hipMemcpyDeviceToHost, st));
    DD_HIP(hipStreamSynchronize(st));
    const unsigned long long biggest = *std::max_element(bins.begin(), bins.end());
    size_t pass_cap = cap;
    if (biggest > pass_cap) {
        // one bin alone is over the budget (one k-mer repeated billions of times lands in one bin): the arrays
        // grow to hold it if the device has the room, otherwise this input cannot be counted here
        pass_cap = (size_t)biggest;
        temp_bytes = dd::exact_sort_temp_bytes(pass_cap, k);
        if ((rc = carve(pass_cap, temp_bytes, counters, hist, lo, lo_alt, hi, hi_alt, temp)))
            return fail(DD_ENOMEM, "exact count: one part of the k-mer space holds %llu k-mers, more than fits in HBM", biggest);
    }
    unsigned long long total = 0;
    int npass = 0;
    for (uint32_t b0 = 0; b0 < (uint32_t)dd::kExactBins;) {
        unsigned long long in_pass = 0;
        uint32_t b1 = b0;
        while (b1 < (uint32_t)dd::kExactBins && in_pass + bins[b1] <= pass_cap) in_pass += bins[b1++];
        if (in_pass) {
            DD_HIP(hipMemsetAsync(counters, 0, 256, st));
            {
                Span sp(c, DD_KERNEL_EXACT);
                dd::launch_kmer_extract(etab_dev, n, max_segments, k, c->canonical, lo, hi, counters, st, 2, hist, b0, b1);
                DD_HIP(hipGetLastError());
                // (every slot below in_pass is written: no sentinel, T^k is an ordinary value here)
                DD_HIP(dd::launch_exact_sort_count(lo, hi, lo_alt, hi_alt, (size_t)in_pass, k, temp, temp_bytes, counters, st));
            }
            unsigned long long h[4] = {0, 0, 0, 0};
            DD_HIP(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));
            if (h[3] != in_pass) return fail(DD_EHIP, "exact count: pass over bins %u..%u appended %llu k-mers, %llu expected", b0, b1, h[3], in_pass);
            total += h[2];
            ++npass;
        }
        b0 = b1;
    }
    c->st_blocks = npass;  // (visible through dd_last_sketch_stats: how many passes the last exact count took)
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

// The driver behind the four schedules: K0 once, then for every k extract (with the genome's index) -> sort -> reduce +
// accumulate, everything at once or in passes over bins of the k-mer space exactly as dd_exact_count_device does.
// out[kk] receives the accumulator's exact_sched_acc_words() counts of k = kmin + kk.
int exact_schedule(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int kmin, int kmax, dd::ExactSched s,
                   const std::vector<uint64_t>& table, std::vector<std::vector<unsigned long long>>& out) {
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
        const size_t tbytes = table.size() * sizeof(uint64_t);
        if ((rc = c->ord.reserve(tbytes))) return rc;
        DD_HIP(hipEventSynchronize(c->stage_free));
        if ((rc = c->stage.reserve(tbytes))) return rc;
        if ((rc = upload(c, c->stage, c->ord.p, table.data(), tbytes, 0))) return rc;
        DD_HIP(hipEventRecord(c->stage_free, st));
        s.table = static_cast<const uint64_t*>(c->ord.p);
    }
    const size_t slots = in.slots, budget = exact_budget();
    const size_t hist_bytes = (size_t)dd::kExactBins * sizeof(unsigned long long);
    int most_passes = 0;
    for (int k = kmin; k <= kmax; ++k) {
        const bool wide = k > 32, sep = dd::exact_tag_mode(k) == 2;
        const size_t arrays = wide ? 4 : 2, per_slot = arrays * sizeof(uint64_t) + (sep ? 2 : 0);
        const bool single = per_slot * slots <= budget;
        size_t cap = single ? slots : std::max<size_t>(budget / per_slot, 4096);   // k-mers per pass
        // workspace for `keys` k-mers: counters (256 B) | bin histogram (32 KiB) | lo | lo_alt [| hi | hi_alt] [| g | g_alt] | sort temp | chunk summaries
        unsigned long long *counters = nullptr, *hist = nullptr;
        uint64_t *lo = nullptr, *lo_alt = nullptr, *hi = nullptr, *hi_alt = nullptr;
        uint8_t *g = nullptr, *g_alt = nullptr;
        void *temp = nullptr, *summaries = nullptr;
        size_t temp_bytes = 0;
        auto carve = [&](size_t keys) -> int {
            const size_t stride = align_up(keys * sizeof(uint64_t), 256), gstride = sep ? align_up(keys, 256) : 0;
            temp_bytes = dd::exact_sched_temp_bytes(keys, k);
            int r = c->exact.reserve(256 + hist_bytes + arrays * stride + 2 * gstride + align_up(temp_bytes, 256) +
                                     dd::exact_sched_scratch_bytes(keys) + 256);
            if (r) return r;
            char* eb = static_cast<char*>(c->exact.p);
            counters = reinterpret_cast<unsigned long long*>(eb);
            hist = reinterpret_cast<unsigned long long*>(eb + 256);
            char* kb = eb + 256 + hist_bytes;
            lo = reinterpret_cast<uint64_t*>(kb);
            lo_alt = reinterpret_cast<uint64_t*>(kb + stride);
            hi = wide ? reinterpret_cast<uint64_t*>(kb + 2 * stride) : nullptr;
            hi_alt = wide ? reinterpret_cast<uint64_t*>(kb + 3 * stride) : nullptr;
            kb += arrays * stride;
            g = sep ? reinterpret_cast<uint8_t*>(kb) : nullptr;
            g_alt = sep ? reinterpret_cast<uint8_t*>(kb + gstride) : nullptr;
            kb += 2 * gstride;
            temp = kb;
            summaries = kb + align_up(temp_bytes, 256);
            return DD_OK;
        };
        const int tag = sep ? 2 : 1;
        DD_HIP(hipMemsetAsync(s.acc, 0, words * sizeof(unsigned long long), st));
        int npass = 0;
        if (single) {
            if ((rc = carve(slots))) return rc;
            Span sp(c, DD_KERNEL_EXACT);
            DD_HIP(hipMemsetAsync(counters, 0, 256, st));
            // unwritten slots: the all-ones key (T^k's run) with genome 0xFF, which sets no bit
            DD_HIP(hipMemsetAsync(lo, 0xFF, slots * sizeof(uint64_t), st));
            if (wide) DD_HIP(hipMemsetAsync(hi, 0xFF, slots * sizeof(uint64_t), st));
            if (sep) DD_HIP(hipMemsetAsync(g, 0xFF, slots, st));
            dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, lo, hi, counters, st, 0, nullptr, 0, 0, tag, g);
            DD_HIP(hipGetLastError());
            dd::ExactSorted sorted{};
            DD_HIP(dd::launch_exact_sort_tagged(lo, hi, lo_alt, hi_alt, g, g_alt, slots, k, temp, temp_bytes, st, &sorted));
            DD_HIP(dd::launch_exact_sched(sorted, slots, k, s, summaries, st));
            npass = 1;
        } else {
            if ((rc = carve(cap))) return rc;
            DD_HIP(hipMemsetAsync(counters, 0, 256 + hist_bytes, st));
            {
                Span sp(c, DD_KERNEL_EXACT);
                dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, lo, hi, counters, st, 1, hist, 0, 0);
            }
            DD_HIP(hipGetLastError());
            std::vector<unsigned long long> bins(dd::kExactBins);
            DD_HIP(hipMemcpyAsync(bins.data(), hist, hist_bytes, hipMemcpyDeviceToHost, st));
            DD_HIP(hipStreamSynchronize(st));
            const unsigned long long biggest = *std::max_element(bins.begin(), bins.end());
            if (biggest > cap) {   // (one bin over the budget: the arrays grow to hold it, as in dd_exact_count_device)
                cap = (size_t)biggest;
                if ((rc = carve(cap)))
                    return fail(DD_ENOMEM, "exact schedule: one part of the k-mer space holds %llu k-mers, more than fits in HBM", biggest);
            }
            for (uint32_t b0 = 0; b0 < (uint32_t)dd::kExactBins;) {
                unsigned long long in_pass = 0;
                uint32_t b1 = b0;
                while (b1 < (uint32_t)dd::kExactBins && in_pass + bins[b1] <= cap) in_pass += bins[b1++];
                if (in_pass) {
                    DD_HIP(hipMemsetAsync(counters, 0, 256, st));
                    {
                        Span sp(c, DD_KERNEL_EXACT);
                        dd::launch_kmer_extract(in.etab_dev, n, in.max_segments, k, c->canonical, lo, hi, counters, st, 2, hist, b0, b1, tag, g);
                        DD_HIP(hipGetLastError());
                        dd::ExactSorted sorted{};
                        DD_HIP(dd::launch_exact_sort_tagged(lo, hi, lo_alt, hi_alt, g, g_alt, (size_t)in_pass, k, temp, temp_bytes, st, &sorted));
                        DD_HIP(dd::launch_exact_sched(sorted, (size_t)in_pass, k, s, summaries, st));
                    }
                    unsigned long long h[4] = {0, 0, 0, 0};
                    DD_HIP(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, st));
                    DD_HIP(hipStreamSynchronize(st));
                    if (h[3] != in_pass) return fail(DD_EHIP, "exact schedule: pass over bins %u..%u appended %llu k-mers, %llu expected", b0, b1, h[3], in_pass);
                    ++npass;
                }
                b0 = b1;
            }
        }
        DD_HIP(hipMemcpyAsync(out[(size_t)(k - kmin)].data(), s.acc, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        DD_HIP(hipStreamSynchronize(st));
        most_passes = std::max(most_passes, npass);
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
    if (ngroups < 1) return fail(DD_EINVAL, "ngroups=%d: at least one group is needed", ngroups);
    if (ngroups > n) return fail(DD_EINVAL, "ngroups=%d is more than the %d leaves", ngroups, n);
    table.assign((size_t)64 + ngroups, 0ull);
    for (int i = 0; i < 64; ++i) table[i] = ~0ull;
    const uint64_t all = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    for (int i = 0; i < n; ++i) {
        if (group[i] < -1 || group[i] >= ngroups) return fail(DD_EINVAL, "group[%d]=%d outside -1..%d", i, group[i], ngroups - 1);
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

int dd_exact_subsets_from_hist(const uint64_t* hist, int n, uint64_t* card) {
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (!hist || !card) return fail(DD_EINVAL, "null argument");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
    return subsets_from_hist(reinterpret_cast<const unsigned long long*>(hist), n, card, 1);
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

// ------------------------------------------------------------------------------- union
int dd_union_device(dd_ctx* c, const uint8_t* const* in_dev, int n, size_t len, uint8_t* out_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || !in_dev || !out_dev) return fail(DD_EINVAL, "bad argument");
    if (len % 16) return fail(DD_EINVAL, "len must be a multiple of 16");
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = c->ptrs.reserve(sizeof(void*) * n))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(sizeof(void*) * n))) return rc;
    if ((rc = upload(c, c->stage, c->ptrs.p, in_dev, sizeof(void*) * n, 0))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, c->stream));
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_union(static_cast<const uint8_t* const*>(c->ptrs.p), n, len, out_dev, c->stream);
    }
    DD_HIP(hipGetLastError());
    return DD_OK;
}

int dd_union(dd_ctx* c, const uint8_t* const* in, int n, size_t len, uint8_t* out) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || !in || !out) return fail(DD_EINVAL, "bad argument");
    if (len % 16) return fail(DD_EINVAL, "len must be a multiple of 16");
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = c->regs.reserve((size_t)(n + 1) * len))) return rc;
    uint8_t* base = static_cast<uint8_t*>(c->regs.p);
    std::vector<const uint8_t*> ptrs(n);
    for (int i = 0; i < n; ++i) {
        DD_HIP(hipMemcpyAsync(base + (size_t)i * len, in[i], len, hipMemcpyHostToDevice, c->stream));
        ptrs[i] = base + (size_t)i * len;
    }
    if ((rc = dd_union_device(c, ptrs.data(), n, len, base + (size_t)n * len))) return rc;
    DD_HIP(hipMemcpyAsync(out, base + (size_t)n * len, len, hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// -------------------------------------------------------------------------------- card
double dd_ertl_mle(const uint32_t hist[64], int log2m) {
    return dd::ertl_mle(hist, log2m, dd::mle_relerr(log2m));
}

int dd_hist_batch_device(dd_ctx* c, const uint8_t* regs_dev, int njobs, uint32_t* hist) {
    if (check_ctx(c)) return DD_EINVAL;
    if (njobs < 0 || (njobs && (!regs_dev || !hist))) return fail(DD_EINVAL, "bad argument");
    if (!njobs) return DD_OK;
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = c->hist.reserve((size_t)njobs * 64 * sizeof(uint32_t)))) return rc;
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_hist(regs_dev, njobs, c->p, static_cast<uint32_t*>(c->hist.p), c->stream);
    }
    DD_HIP(hipGetLastError());
    DD_HIP(hipMemcpyAsync(hist, c->hist.p, (size_t)njobs * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

int dd_card_batch_device(dd_ctx* c, const uint8_t* regs_dev, int njobs, double* est) {
    if (check_ctx(c)) return DD_EINVAL;
    if (njobs < 0 || (njobs && (!regs_dev || !est))) return fail(DD_EINVAL, "bad argument");
    if (!njobs) return DD_OK;
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = c->hist.reserve((size_t)njobs * 64 * sizeof(uint32_t)))) return rc;
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_hist(regs_dev, njobs, c->p, static_cast<uint32_t*>(c->hist.p), c->stream);
    }
    DD_HIP(hipGetLastError());
    return estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), (size_t)njobs, est);
}

int dd_card_batch(dd_ctx* c, const uint8_t* regs, int njobs, double* est) {
    if (check_ctx(c)) return DD_EINVAL;
    if (njobs < 0 || (njobs && (!regs || !est))) return fail(DD_EINVAL, "bad argument");
    if (!njobs) return DD_OK;
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)njobs << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, regs, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_card_batch_device(c, static_cast<const uint8_t*>(c->regs.p), njobs, est);
}

int dd_card(dd_ctx* c, const uint8_t* regs, double* est) { return dd_card_batch(c, regs, 1, est); }

// ------------------------------------------------------------------------- progressive
int dd_progressive_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, const int32_t* orderings,
                          int norder, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || norder < 1 || !leaf_dev || !orderings || !card)
        return fail(DD_EINVAL, "bad argument");
    for (size_t i = 0; i < (size_t)norder * n; ++i)
        if (orderings[i] < 0 || orderings[i] >= n) return fail(DD_EINVAL, "ordering entry %d outside 0..%d", orderings[i], n - 1);
    DeviceGuard guard(c->device);
    const size_t njobs = (size_t)norder * n * K;
    int rc;
    if ((rc = c->hist.reserve(njobs * 64 * sizeof(uint32_t)))) return rc;
    if ((rc = c->ord.reserve(sizeof(int32_t) * norder * n))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(sizeof(int32_t) * norder * n))) return rc;
    if ((rc = upload(c, c->stage, c->ord.p, orderings, sizeof(int32_t) * norder * n, 0))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, c->stream));
    {
        Span sp(c, DD_KERNEL_UNION);
        // bit-plane AND-scan (dd_pscan.hip) where it applies; DD_PROGRESSIVE_STREAM=1 keeps the streaming kernel of
        // dd_union.hip (one LDS atomic per register per prefix) for A/B runs and for the equality test
        bool done = false;
        if (dd::pscan_usable(n, norder, c->p) && !getenv("DD_PROGRESSIVE_STREAM")) {
            if ((rc = c->gram.reserve(dd::pscan_scratch_bytes(n, K, c->p, norder)))) return rc;
            dd::launch_register_range(leaf_dev, n, K, c->p, static_cast<uint32_t*>(c->gram.p), c->stream);
            std::vector<uint32_t> rng((size_t)K * 2);   // (which thresholds exist decides the tile size: 296 bytes back to the host)
            DD_HIP(hipMemcpyAsync(rng.data(), c->gram.p, rng.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            DD_HIP(hipStreamSynchronize(c->stream));
            done = dd::launch_progressive_pscan(leaf_dev, n, K, c->p, static_cast<const int32_t*>(c->ord.p), norder, rng.data(), c->gram.p,
                                                static_cast<uint32_t*>(c->hist.p), c->stream);
        }
        c->k2_path = done ? DD_K2_PROGRESSIVE_PSCAN : DD_K2_PROGRESSIVE_STREAM;
        if (!done)
            dd::launch_progressive(leaf_dev, n, K, c->p, static_cast<const int32_t*>(c->ord.p), norder,
                                   static_cast<uint32_t*>(c->hist.p), c->stream);
    }
    DD_HIP(hipGetLastError());
    return estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), njobs, card);
}

int dd_progressive(dd_ctx* c, const uint8_t* leaf, int n, int K, const int32_t* orderings, int norder,
                   double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_progressive_device(c, static_cast<const uint8_t*>(c->regs.p), n, K, orderings, norder, card);
}

// ---------------------------------------------------------------------------- pairwise
int dd_pairwise_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf_dev || !card) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t njobs = (size_t)n * n * K;
    int rc;
    if ((rc = c->hist.reserve(njobs * 64 * sizeof(uint32_t)))) return rc;
    // all pairs as int8 Gram matrices on the matrix cores (dd_gram.hip); DD_PAIRWISE_STREAM=1 keeps the streaming
    // kernel of dd_union.hip (one LDS atomic per register per pair) for A/B runs and for the equality test
    const bool gram = dd::gram_usable(n, c->p) && !getenv("DD_PAIRWISE_STREAM");
    if (gram && (rc = c->gram.reserve(dd::gram_scratch_bytes(n, K, c->p, nullptr)))) return rc;
    c->k2_path = gram ? DD_K2_PAIRWISE_GRAM : DD_K2_PAIRWISE_STREAM;
    {
        Span sp(c, DD_KERNEL_UNION);
        if (gram) {
            DD_HIP(hipMemsetAsync(c->hist.p, 0, njobs * 64 * sizeof(uint32_t), c->stream));
            dd::launch_pairwise_gram(leaf_dev, n, K, c->p, static_cast<uint32_t*>(c->hist.p), c->gram.p, c->stream);
        } else {
            dd::launch_pairwise(leaf_dev, n, K, c->p, static_cast<uint32_t*>(c->hist.p), c->stream);
        }
    }
    DD_HIP(hipGetLastError());
    // lower triangle histograms are all-zero: give them the mirrored estimate afterwards
    std::vector<double> tmp(njobs);
    if ((rc = c->est.reserve(njobs * sizeof(double)))) return rc;
    // only the upper triangle (i <= j) holds real histograms; estimate everything on the device
    // would waste work on empty ones, so fill empties with m in bin 0 -> estimate 0 cheaply
    dd::launch_mle(static_cast<const uint32_t*>(c->hist.p), njobs, c->p, static_cast<double*>(c->est.p),
                   c->stream);
    DD_HIP(hipGetLastError());
    DD_HIP(hipMemcpyAsync(tmp.data(), c->est.p, njobs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int a = i <= j ? i : j, b = i <= j ? j : i;
            memcpy(card + ((size_t)i * n + j) * K, tmp.data() + ((size_t)a * n + b) * K, sizeof(double) * K);
        }
    return DD_OK;
}

int dd_pairwise(dd_ctx* c, const uint8_t* leaf, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_pairwise_device(c, static_cast<const uint8_t*>(c->regs.p), n, K, card);
}

// -------------------------------------------------------------------------- leave-out
int dd_leave_out_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, const int32_t* group, int ngroups, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf_dev || !group || !card) return fail(DD_EINVAL, "bad argument");
    if (ngroups < 1) return fail(DD_EINVAL, "ngroups=%d: at least one group is needed", ngroups);
    if (ngroups > n) return fail(DD_EINVAL, "ngroups=%d is more than the %d leaves", ngroups, n);
    for (int i = 0; i < n; ++i)
        if (group[i] < -1 || group[i] >= ngroups) return fail(DD_EINVAL, "group[%d]=%d outside -1..%d", i, group[i], ngroups - 1);
    // the kernel's slot table: leaves ordered by group (the floor, -1, first), the last slot of each group carrying its id
    std::vector<int> start(ngroups + 2, 0);          // slots of group g: [start[g + 1], start[g + 2])
    for (int i = 0; i < n; ++i) ++start[group[i] + 2];
    for (int g = 0; g < ngroups; ++g)
        if (start[g + 2] == n) return fail(DD_EINVAL, "group %d holds every leaf: the union of the rest is empty", g);
    for (int s = 1; s <= ngroups + 1; ++s) start[s] += start[s - 1];
    std::vector<int32_t> tab((size_t)2 * n);
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i) {
        const int j = fill[group[i] + 1]++;
        tab[2 * j] = i;
        tab[2 * j + 1] = (j + 1 == start[group[i] + 2]) ? group[i] : -2;
    }
    DeviceGuard guard(c->device);
    const int nslots = (int)(tab.size() / 2);
    const size_t njobs = (size_t)(ngroups + 1) * K;
    int rc;
    if ((rc = c->hist.reserve(njobs * 64 * sizeof(uint32_t)))) return rc;
    if ((rc = c->ord.reserve(sizeof(int32_t) * tab.size()))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(sizeof(int32_t) * tab.size()))) return rc;
    if ((rc = upload(c, c->stage, c->ord.p, tab.data(), sizeof(int32_t) * tab.size(), 0))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, c->stream));
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_leaveout(leaf_dev, K, c->p, static_cast<const int32_t*>(c->ord.p), nslots, ngroups,
                            static_cast<uint32_t*>(c->hist.p), c->stream);
    }
    DD_HIP(hipGetLastError());
    return estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), njobs, card);
}

int dd_leave_out(dd_ctx* c, const uint8_t* leaf, int n, int K, const int32_t* group, int ngroups, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_leave_out_device(c, static_cast<const uint8_t*>(c->regs.p), n, K, group, ngroups, card);
}

// ------------------------------------------------------------------------ all subsets
// dd_subsets.hip: every subset's histogram from threshold bit planes.  Columns are taken Kc at a time so that the
// histograms (2^n Kc 64 u32) stay within 256 MiB and the partial counts within 512 MiB.
int dd_subsets_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (K < 1 || !leaf_dev || !card) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t nsub = (size_t)1 << n;
    const int Kc = (int)std::min<size_t>((size_t)K, std::max<size_t>(1, ((size_t)256 << 20) / (nsub * 64 * sizeof(uint32_t))));
    const size_t part_budget = (size_t)512 << 20;
    int rc;
    if ((rc = c->gram.reserve((size_t)K * 2 * sizeof(uint32_t)))) return rc;
    if ((rc = c->hist.reserve(nsub * Kc * 64 * sizeof(uint32_t)))) return rc;
    std::vector<uint32_t> rng((size_t)K * 2);
    dd::launch_register_range(leaf_dev, n, K, c->p, static_cast<uint32_t*>(c->gram.p), c->stream);
    DD_HIP(hipMemcpyAsync(rng.data(), c->gram.p, rng.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    // the workgroup tables of every chunk after the ranges, one upload
    std::vector<dd::SubsetsPlan> plans;
    std::vector<int32_t> tab(rng.begin(), rng.end());
    std::vector<size_t> wg_off;
    size_t part_bytes = 0;
    for (int k0 = 0; k0 < K; k0 += Kc) {
        plans.push_back(dd::plan_subsets(n, c->p, rng.data(), k0, std::min(Kc, K - k0), part_budget));
        wg_off.push_back(tab.size());
        tab.insert(tab.end(), plans.back().wg.begin(), plans.back().wg.end());
        part_bytes = std::max(part_bytes, plans.back().part_bytes);
    }
    if ((rc = c->gram.reserve(part_bytes))) return rc;
    if ((rc = c->ord.reserve(sizeof(int32_t) * tab.size()))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(sizeof(int32_t) * tab.size()))) return rc;
    if ((rc = upload(c, c->stage, c->ord.p, tab.data(), sizeof(int32_t) * tab.size(), 0))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, c->stream));
    const uint32_t* rng_dev = static_cast<const uint32_t*>(c->ord.p);
    uint32_t* part_dev = static_cast<uint32_t*>(c->gram.p);
    std::vector<double> est;
    for (size_t i = 0; i < plans.size(); ++i) {
        const int k0 = (int)i * Kc, kc = std::min(Kc, K - k0);
        {
            Span sp(c, DD_KERNEL_UNION);
            dd::launch_subsets(leaf_dev, n, K, c->p, k0, kc, plans[i], static_cast<const int32_t*>(c->ord.p) + wg_off[i], rng_dev,
                               part_dev, static_cast<uint32_t*>(c->hist.p), c->stream);
        }
        DD_HIP(hipGetLastError());
        est.resize(nsub * kc);
        if ((rc = estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), nsub * kc, est.data()))) return rc;
        for (size_t s = 0; s < nsub; ++s) memcpy(card + s * K + k0, est.data() + s * kc, sizeof(double) * kc);
    }
    for (int kk = 0; kk < K; ++kk) card[kk] = 0.0;   // the empty set
    return DD_OK;
}

int dd_subsets(dd_ctx* c, const uint8_t* leaf, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (K < 1 || !leaf) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_subsets_device(c, static_cast<const uint8_t*>(c->regs.p), n, K, card);
}

// ---------------------------------------------------------------------- extend / greedy
namespace {

// one dd_extend step: cards of base U leaf[rows[r]] (base_dev null: of the rows themselves) -> card[nrows][K] on the host
int extend_step(dd_ctx* c, const uint8_t* base_dev, const uint8_t* leaf_dev, int K, const int32_t* rows, int nrows, double* card) {
    const size_t njobs = (size_t)nrows * K;
    int rc;
    if ((rc = c->hist.reserve((njobs + K) * 64 * sizeof(uint32_t)))) return rc;
    if ((rc = c->ord.reserve(sizeof(int32_t) * nrows))) return rc;
    DD_HIP(hipEventSynchronize(c->stage_free));
    if ((rc = c->stage.reserve(sizeof(int32_t) * nrows))) return rc;
    if ((rc = upload(c, c->stage, c->ord.p, rows, sizeof(int32_t) * nrows, 0))) return rc;
    DD_HIP(hipEventRecord(c->stage_free, c->stream));
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_extend(base_dev, leaf_dev, K, c->p, static_cast<const int32_t*>(c->ord.p), nrows, static_cast<uint32_t*>(c->hist.p),
                          c->stream);
    }
    DD_HIP(hipGetLastError());
    return estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), njobs, card);
}

int extend_args(dd_ctx* c, const uint8_t* leaf, int n, int K, const int32_t* rows, int nrows, const double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf || !card) return fail(DD_EINVAL, "bad argument");
    if (nrows < 1) return fail(DD_EINVAL, "nrows=%d: at least one row is needed", nrows);
    if (rows)
        for (int r = 0; r < nrows; ++r)
            if (rows[r] < 0 || rows[r] >= n) return fail(DD_EINVAL, "rows[%d]=%d outside 0..%d", r, rows[r], n - 1);
    return DD_OK;
}

int greedy_args(dd_ctx* c, const uint8_t* leaf, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps,
                const int32_t* order, const double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf || !cand || !order || !card) return fail(DD_EINVAL, "bad argument");
    if (kmin < 1 || kmin + K - 1 > 64) return fail(DD_EINVAL, "k window %d..%d outside 1..64", kmin, kmin + K - 1);
    if (mode != DD_GREEDY_MAX && mode != DD_GREEDY_MIN) return fail(DD_EINVAL, "mode=%d: DD_GREEDY_MAX (0) or DD_GREEDY_MIN (1)", mode);
    if (ncand < 1 || ncand > n) return fail(DD_EINVAL, "ncand=%d outside 1..%d", ncand, n);
    std::vector<char> seen(n, 0);
    for (int i = 0; i < ncand; ++i) {
        if (cand[i] < 0 || cand[i] >= n) return fail(DD_EINVAL, "cand[%d]=%d outside 0..%d", i, cand[i], n - 1);
        if (seen[cand[i]]) return fail(DD_EINVAL, "cand[%d]=%d is a repeat: candidates are distinct", i, cand[i]);
        seen[cand[i]] = 1;
    }
    if (nfixed < 0 || nfixed > nsteps) return fail(DD_EINVAL, "nfixed=%d outside 0..nsteps=%d", nfixed, nsteps);
    if (nsteps < 1 || nsteps > ncand) return fail(DD_EINVAL, "nsteps=%d outside 1..ncand=%d", nsteps, ncand);
    return DD_OK;
}

// the selection rule of include/dandd_hip.h: the largest card / k of the window, a later k winning a tie
double window_delta(const double* card, int K, int kmin) {
    double best = 0.0;
    for (int kk = 0; kk < K; ++kk) {
        const double v = card[kk] / (double)(kmin + kk);
        if (best <= v) best = v;
    }
    return best;
}

}  // namespace

int dd_extend_device(dd_ctx* c, const uint8_t* base_dev, const uint8_t* leaf_dev, int n, int K, const int32_t* rows, int nrows,
                     double* card) {
    int rc;
    if (!rows) nrows = n;
    if ((rc = extend_args(c, leaf_dev, n, K, rows, nrows, card))) return rc;
    if ((uintptr_t)base_dev % 16) return fail(DD_EINVAL, "base must be 16-byte aligned");
    std::vector<int32_t> all;
    if (!rows) {
        all.resize(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        rows = all.data();
    }
    DeviceGuard guard(c->device);
    return extend_step(c, base_dev, leaf_dev, K, rows, nrows, card);
}

int dd_extend(dd_ctx* c, const uint8_t* base, const uint8_t* leaf, int n, int K, const int32_t* rows, int nrows, double* card) {
    int rc;
    if (!rows) nrows = n;
    if ((rc = extend_args(c, leaf, n, K, rows, nrows, card))) return rc;
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p, one = (size_t)K << c->p;
    if ((rc = c->regs.reserve(bytes + (base ? one : 0)))) return rc;
    uint8_t* dev = static_cast<uint8_t*>(c->regs.p);
    DD_HIP(hipMemcpyAsync(dev, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    if (base) DD_HIP(hipMemcpyAsync(dev + bytes, base, one, hipMemcpyHostToDevice, c->stream));
    return dd_extend_device(c, base ? dev + bytes : nullptr, dev, n, K, rows, nrows, card);
}

int dd_greedy_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed,
                     int nsteps, int32_t* order, double* card) {
    int rc;
    if ((rc = greedy_args(c, leaf_dev, n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card))) return rc;
    DeviceGuard guard(c->device);
    const size_t one = (size_t)K << c->p;
    if ((rc = c->gram.reserve(one))) return rc;          // the running union: it never leaves the device
    uint8_t* base = static_cast<uint8_t*>(c->gram.p);
    std::vector<int32_t> left(cand + nfixed, cand + ncand);   // in tie-break order throughout
    std::vector<double> cards((size_t)ncand * K);
    for (int j = 0; j < nsteps; ++j) {
        const bool given = j < nfixed;
        const int32_t* rows = given ? cand + j : left.data();
        const int nrows = given ? 1 : (int)left.size();
        if ((rc = extend_step(c, j ? base : nullptr, leaf_dev, K, rows, nrows, cards.data()))) return rc;
        int pick = 0;
        double best = window_delta(cards.data(), K, kmin);
        for (int r = 1; r < nrows; ++r) {
            const double d = window_delta(cards.data() + (size_t)r * K, K, kmin);
            if (mode == DD_GREEDY_MAX ? d > best : d < best) best = d, pick = r;
        }
        order[j] = rows[pick];
        memcpy(card + (size_t)j * K, cards.data() + (size_t)pick * K, sizeof(double) * K);
        if (!given) left.erase(left.begin() + pick);
        if (j + 1 == nsteps) break;
        const uint8_t* row = leaf_dev + (size_t)order[j] * one;
        Span sp(c, DD_KERNEL_UNION);
        if (j == 0)
            DD_HIP(hipMemcpyAsync(base, row, one, hipMemcpyDeviceToDevice, c->stream));
        else
            dd::launch_extend_fold(base, row, one, c->stream);
        DD_HIP(hipGetLastError());
    }
    return DD_OK;
}

int dd_greedy(dd_ctx* c, const uint8_t* leaf, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps,
              int32_t* order, double* card) {
    int rc;
    if ((rc = greedy_args(c, leaf, n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card))) return rc;
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    if ((rc = c->regs.reserve(bytes))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return dd_greedy_device(c, static_cast<const uint8_t*>(c->regs.p), n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card);
}

// ------------------------------------------------------------------------- measurement
int dd_timing_enable(dd_ctx* c, int on) {
    if (check_ctx(c)) return DD_EINVAL;
    c->timing = on != 0;
    return DD_OK;
}

int dd_timing_reset(dd_ctx* c) {
    if (check_ctx(c)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    DD_HIP(hipStreamSynchronize(c->stream));
    for (auto& v : c->spans) {
        for (auto& s : v) {
            c->pool.push_back(s.a);
            c->pool.push_back(s.b);
        }
        v.clear();
    }
    return DD_OK;
}

int dd_timing_read(dd_ctx* c, int which, double* total_ms, int* launches) {
    if (check_ctx(c)) return DD_EINVAL;
    if (which < 0 || which >= DD_KERNEL_COUNT) return fail(DD_EINVAL, "bad kernel id %d", which);
    DeviceGuard guard(c->device);
    DD_HIP(hipStreamSynchronize(c->stream));
    double tot = 0;
    for (auto& s : c->spans[which]) {
        float ms = 0;
        DD_HIP(hipEventElapsedTime(&ms, s.a, s.b));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int)c->spans[which].size();
    return DD_OK;
}

int dd_last_sketch_stats(dd_ctx* c, uint64_t* tokens, uint64_t* updates, int* sweep_blocks) {
    if (check_ctx(c)) return DD_EINVAL;
    if (tokens) *tokens = c->st_tokens;
    if (updates) *updates = c->st_updates;
    if (sweep_blocks) *sweep_blocks = c->st_blocks;
    return DD_OK;
}

int dd_last_k2_path(dd_ctx* c) {
    if (check_ctx(c)) return DD_EINVAL;
    return c->k2_path;
}

// --------------------------------------------------------------------------- synthetic
long dd_plan_sweep(int log2m, const size_t* nbytes, int ngenomes, int kmin, int kmax, dd_plan_job* out,
                   long cap) {
    if (log2m < 4 || log2m > 20) return fail(DD_EINVAL, "log2m %d outside 4..20", log2m);
    if (ngenomes < 0 || (ngenomes && !nbytes) || cap < 0 || (cap && !out)) return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    const std::vector<dd::SweepClass> classes =
        dd::plan_sweep(log2m, 1, nbytes, ngenomes, kmin, kmax, dd::PlanKnobs::from_env());
    long n = 0;
    for (const dd::SweepClass& sc : classes) {
        for (const dd::SweepJob& j : sc.jobs) {
            if (n < cap)
                out[n] = dd_plan_job{sc.kclass, sc.plan.mode, sc.plan.lds_bytes, j.genome, j.kfirst, j.nk,
                                     j.tile_begin, j.tile_end, j.slice};
            ++n;
        }
    }
    return n;
}

size_t dd_synth_size(uint64_t nbases, int nrec) {
    if (nrec < 1) return 0;
    return dd::synth_size(nbases, nrec);
}

int dd_synth_fasta_device(dd_ctx* c, uint64_t seed, int genome_index, uint64_t nbases, int nrec,
                          uint8_t* out_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (nrec < 1 || nrec > 65535 || genome_index < 0 || genome_index > 65535 || !out_dev)
        return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    dd::launch_synth(seed, genome_index, nbases, nrec, out_dev, c->stream);
    DD_HIP(hipGetLastError());
    return DD_OK;
}

size_t dd_synth_realistic_size(uint64_t seed, uint64_t nbases) {
    if (!nbases) return 0;
    const std::vector<uint64_t> tab = dd::synth_realistic_table(seed, nbases);
    return (size_t)tab[tab.size() - 2];
}

int dd_synth_realistic_device(dd_ctx* c, uint64_t seed, int genome_index, uint64_t nbases, uint8_t* out_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (genome_index < 0 || genome_index > 65535 || !out_dev) return fail(DD_EINVAL, "bad argument");
    if (!nbases) return DD_OK;
    DeviceGuard guard(c->device);
    const std::vector<uint64_t> tab = dd::synth_realistic_table(seed, nbases);
    int rc;
    if ((rc = c->synth.reserve(tab.size() * sizeof(uint64_t)))) return rc;
    DD_HIP(hipMemcpyAsync(c->synth.p, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));   // (`tab` is pageable host memory about to go out of scope)
    dd::launch_synth_realistic(seed, genome_index, static_cast<const uint64_t*>(c->synth.p), (uint32_t)(tab.size() / 2 - 1),
                               tab[tab.size() - 2], out_dev, c->stream);
    DD_HIP(hipGetLastError());
    return DD_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------- multi-GPU: RCCL over xGMI behind the C ABI
// (genome x k) jobs shard over the GPUs of a node with no data-path exchange; what crosses xGMI is the root --
// every rank's [K][m] slab of byte-max-merged registers through ncclAllReduce(ncclUint8, ncclMax) -- and, for the schedules that
// need every leaf (progressive, kij), one ncclAllGather of the ranks' leaf slabs.  The reference's only parallelism is
// `parallel -j 95%` over k on one host (/root/reference/lib/huffman_dandd.py:217).  librccl is opened at the first dd_comm_*
// call (the copy already mapped into the process if there is one -- PyTorch-ROCm brings its own), never linked: a single-GPU
// user of this library needs no RCCL.
#include <rccl/rccl.h>
namespace {
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};
RcclApi* rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // DD_RCCL_LIB names THE copy to use (nothing else is tried when it is set)
        const char* named = getenv("DD_RCCL_LIB");
        const char* names[] = {named, named ? nullptr : "librccl.so.1", named ? nullptr : "librccl.so", named ? nullptr : "/opt/rocm/lib/librccl.so.1"};
        for (int pass = 0; pass < 2 && !api.lib; ++pass)      // pass 0: a copy that is already mapped (RTLD_NOLOAD)
            for (const char* n : names)
                if (n && !api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
        if (!api.lib) {
            const char* e = dlerror();                        // one call: dlerror() clears its state when read
            api.why = std::string("librccl.so not found (") + (e ? e : "?") + "); set DD_RCCL_LIB";
            return;
        }
        auto sym = [&](const char* n) {
            void* f = dlsym(api.lib, n);
            if (!f && api.why.empty()) api.why = std::string("librccl: no symbol ") + n;
            return f;
        };
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(sym("ncclAllReduce"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    });
    return &api;
}
int rccl_ready(RcclApi*& api) {
    api = rccl();
    if (!api->why.empty()) return fail(DD_ENODEV, "RCCL: %s", api->why.c_str());
    return DD_OK;
}
#define DD_RCCL(api, expr)                                                                                     \
    do {                                                                                                       \
        const ncclResult_t r_ = (expr);                                                                        \
        if (r_ != ncclSuccess) return fail(DD_EHIP, "RCCL: %s failed: %s", #expr, (api)->GetErrorString(r_)); \
    } while (0)
}  // namespace

static_assert(DD_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "dandd_hip.h: DD_COMM_ID_BYTES is ncclUniqueId's size");

int dd_comm_unique_id(uint8_t* id) {
    if (!id) return fail(DD_EINVAL, "null argument");
    RcclApi* api;
    int rc;
    if ((rc = rccl_ready(api))) return rc;
    ncclUniqueId u;
    DD_RCCL(api, api->GetUniqueId(&u));
    memcpy(id, u.internal, DD_COMM_ID_BYTES);
    return DD_OK;
}

int dd_comm_init(dd_ctx* c, int rank, int world, const uint8_t* id) {
    if (check_ctx(c)) return DD_EINVAL;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(DD_EINVAL, "rank %d of %d", rank, world);
    if (c->comm) return fail(DD_EINVAL, "this context already belongs to a communicator (dd_comm_destroy first)");
    RcclApi* api;
    int rc;
    if ((rc = rccl_ready(api))) return rc;
    DeviceGuard guard(c->device);   // ncclCommInitRank binds the communicator to the CURRENT device: the context's
    ncclUniqueId u;
    memcpy(u.internal, id, DD_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    DD_RCCL(api, api->CommInitRank(&comm, world, u, rank));
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_world = world;
    c->comm_calls[0] = c->comm_calls[1] = 0;
    return DD_OK;
}

int dd_comm_destroy(dd_ctx* c) {
    if (!c) return DD_EINVAL;
    if (!c->comm) return DD_OK;
    RcclApi* api = rccl();
    DeviceGuard guard(c->device);
    (void)hipStreamSynchronize(c->stream);
    const ncclResult_t r = api->CommDestroy ? api->CommDestroy(static_cast<ncclComm_t>(c->comm)) : ncclSuccess;
    c->comm = nullptr;
    c->comm_rank = 0;
    c->comm_world = 1;
    return r == ncclSuccess ? DD_OK : fail(DD_EHIP, "RCCL: ncclCommDestroy failed");
}

int dd_comm_info(dd_ctx* c, int* rank, int* world, unsigned long long* allreduces, unsigned long long* allgathers) {
    if (check_ctx(c)) return DD_EINVAL;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm ? c->comm_world : 0;   // 0: no communicator
    if (allreduces) *allreduces = c->comm_calls[0];
    if (allgathers) *allgathers = c->comm_calls[1];
    return DD_OK;
}

int dd_allreduce_max_u8(dd_ctx* c, uint8_t* regs_dev, size_t n) {
    if (check_ctx(c)) return DD_EINVAL;
    if (!c->comm) return fail(DD_EINVAL, "no communicator on this context (dd_comm_init)");
    if (n && !regs_dev) return fail(DD_EINVAL, "null argument");
    if (!n) return DD_OK;
    RcclApi* api = rccl();
    DeviceGuard guard(c->device);
    DD_RCCL(api, api->AllReduce(regs_dev, regs_dev, n, ncclUint8, ncclMax, static_cast<ncclComm_t>(c->comm), c->stream));
    ++c->comm_calls[0];
    return DD_OK;
}

int dd_allgather_u8(dd_ctx* c, const uint8_t* send_dev, size_t n, uint8_t* recv_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (!c->comm) return fail(DD_EINVAL, "no communicator on this context (dd_comm_init)");
    if (n && (!send_dev || !recv_dev)) return fail(DD_EINVAL, "null argument");
    if (!n) return DD_OK;
    RcclApi* api = rccl();
    DeviceGuard guard(c->device);
    DD_RCCL(api, api->AllGather(send_dev, recv_dev, n, ncclUint8, static_cast<ncclComm_t>(c->comm), c->stream));
    ++c->comm_calls[1];
    return DD_OK;
}
