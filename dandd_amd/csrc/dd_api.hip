// dd_api.hip -- the C ABI of libdandd_hip.so (declared in include/dandd_hip.h).
//
// Host-side orchestration only: workspace management in HBM, job tables for the sweep,
// stream/event plumbing.  Every entry point names the DandD command line it replaces in
// include/dandd_hip.h.  There is no CPU fallback anywhere in this file.  Here: context, sketch, timing
// and stats, synth, comm.  Union, card and the HLL schedules are in dd_k2_api.hip, the exact count and
// schedules in dd_exact_api.hip, the file-ingestion pipeline (dd_sketch_fasta, dd_sketch_files,
// dd_inflate_files) in dd_ingest.hip; the helpers they share are in dd_ctx.h.
#include <memory>
#include <mutex>
#include "dd_ctx.h"

using dd::FileBuf;

thread_local std::string g_err;   // (declared in dd_ctx.h)


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
    std::vector<dd::PackGenome> ptab;
    size_t max_chunks = 0;
    int rc;
    if ((rc = layout_tokens(c, fasta_dev, nbytes, ngenomes, ptab, max_chunks))) return rc;

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
    uint64_t tokens_ub = 0;
    for (int g = 0; g < ngenomes; ++g) {
        const dd::TokenStream& ts = ptab[g].out;
        gtab[g] = dd::SweepGenome{ts.codes, ts.bad, ts.ntok, regs_dev + (size_t)g * K * m,
                                  bitmap_base ? bitmap_base + (size_t)g * dd::kBitmapStride : nullptr,
                                  bigmap_base ? bigmap_base + (size_t)g * bigmap_stride : nullptr};
        tokens_ub += nbytes[g];
    }

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
        // the first epoch's updates of rho = 1: one bit per register instead of a record each (dd_scatter.hip,
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
