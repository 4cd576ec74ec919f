// dd_sketch_api.hip -- the sketch entry points of the C ABI (dd_sketch_device, dd_sketch_buffer): K0, then the K1 classes
// of the call's plan (dd_plan.h).  Every sketch goes through dd_sketch_device: the ingestion pipeline's batches too.
#include "dd_ctx.h"

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

// Fork and join on the side streams: run() gives `launch` the next lane, behind the mark `side_go` on the caller's stream,
// and puts the caller's stream behind what the lane was given -- or, without `fork`, gives it the caller's stream.  With
// `join_now` false the caller's stream is put behind the lane only by join(): what the caller's stream is given in between runs
// beside the lane.
struct SideLanes {
    dd_ctx* c;
    int lane = 0, joined = 0;
    template <class F>
    int run(bool fork, F&& launch, bool join_now = true) {
        const int l = lane & 7;
        if (!fork) return launch(c->stream), DD_OK;
        // (the lane's mark is recorded whatever the wait returned, so that join() never waits on the mark of an earlier call)
        const hipError_t waited = hipStreamWaitEvent(c->side[l], c->side_go, 0);
        if (waited == hipSuccess) launch(c->side[l]);
        const hipError_t marked = hipEventRecord(c->side_done[l], c->side[l]);
        ++lane;
        DD_HIP(waited);
        DD_HIP(marked);
        return join_now ? join() : DD_OK;
    }
    int join() {
        for (; joined < lane; ++joined) DD_HIP(hipStreamWaitEvent(c->stream, c->side_done[joined & 7], 0));
        return DD_OK;
    }
};

// The presence-bitmap workspaces of a call, reserved and zeroed: for the small-k class (k <= 9) and for k = 10 (, 11) at
// log2m >= 19 (dd_kernels.h).  Genome g's are at small + g * kBitmapStride and big + g * big_stride; null: class not planned.
// sat (sat_words of them, 0: none): the call's saturation flags (dd_kernels.h), one per row, behind the small bitmaps in the same
// allocation and zeroed by the same memset -- by one of their own only in a call that has flags and no small-k class.
struct Bitmaps { uint32_t* small = nullptr; uint32_t* big = nullptr; size_t big_stride = 0; uint32_t* sat = nullptr; };
static int reserve_bitmaps(dd_ctx* c, const dd::PlanKnobs& knobs, const size_t* nbytes, int ngenomes, int kmin, int kmax, size_t sat_words, Bitmaps& bm) {
    int rc, ka = 0, kb = 0;
    if (kmin <= dd::kBitmapMaxK || sat_words) {
        const size_t words = kmin <= dd::kBitmapMaxK ? (size_t)ngenomes * dd::kBitmapStride : 0, bbytes = (words + sat_words) * sizeof(uint32_t);
        if ((rc = c->bitmaps.reserve(bbytes))) return rc;
        if (words) bm.small = static_cast<uint32_t*>(c->bitmaps.p);
        if (sat_words) bm.sat = static_cast<uint32_t*>(c->bitmaps.p) + words;
        DD_HIP(hipMemsetAsync(c->bitmaps.p, 0, bbytes, c->stream));
    }
    if (dd::plan_bigmap_range(c->p, kmin, kmax, knobs, nbytes, ngenomes, &ka, &kb)) {
        bm.big_stride = dd::bigmap_offset_words(kb + 1, c->canonical != 0);
        const size_t bbytes = (size_t)ngenomes * bm.big_stride * sizeof(uint32_t);
        if ((rc = c->bigmaps.reserve(bbytes))) return rc;
        bm.big = static_cast<uint32_t*>(c->bigmaps.p);
        DD_HIP(hipMemsetAsync(bm.big, 0, bbytes, c->stream));
    }
    return DD_OK;
}

// The call's K1 job tables (dd_plan.hip): the cached entry for these sizes, k range and knobs, or a new plan, uploaded through
// `stage`, in place of the least recently used one.  The entry being replaced may still be read by kernels of an earlier
// call: its device table is only ever written by copies on this same stream, and a table that must grow is freed by
// hipFree, which waits.
static int cached_plan(dd_ctx* c, StageSet& stage, const dd::PlanKnobs& knobs, const size_t* nbytes, int ngenomes, int kmin, int kmax, dd_ctx::PlanEntry** out) {
    dd_ctx::PlanEntry* pc = &c->plans[0];
    for (auto& pe : c->plans) {
        if (pe.valid && pe.kmin == kmin && pe.kmax == kmax && pe.knobs == knobs && pe.sizes.size() == (size_t)ngenomes &&
            std::equal(pe.sizes.begin(), pe.sizes.end(), nbytes)) {
            pe.last_use = ++c->plan_clock;
            *out = &pe;
            return DD_OK;
        }
        if (pe.last_use < pc->last_use) pc = &pe;
    }
    pc->last_use = ++c->plan_clock;
    pc->valid = false;
    pc->classes = dd::plan_sweep(c->p, c->canonical, nbytes, ngenomes, kmin, kmax, knobs);
    size_t job_bytes = 0;
    pc->job_off.assign(pc->classes.size(), 0);
    for (size_t i = 0; i < pc->classes.size(); ++i) {
        pc->job_off[i] = job_bytes;
        job_bytes += align_up(sizeof(dd::SweepJob) * pc->classes[i].jobs.size(), 256);
    }
    int rc;
    if ((rc = pc->jobtab.reserve(job_bytes))) return rc;
    if ((rc = stage.jobs.reserve(job_bytes))) return rc;
    for (size_t i = 0; i < pc->classes.size(); ++i)
        if ((rc = upload(c, stage.jobs, static_cast<char*>(pc->jobtab.p) + pc->job_off[i], pc->classes[i].jobs.data(),
                         sizeof(dd::SweepJob) * pc->classes[i].jobs.size(), pc->job_off[i])))
            return rc;
    pc->kmin = kmin;
    pc->kmax = kmax;
    pc->knobs = knobs;
    pc->sizes.assign(nbytes, nbytes + ngenomes);
    pc->valid = true;
    *out = pc;
    return DD_OK;
}

// Bucket mode (log2m >= 17): c->buckets laid out by dd::bucket_layout, its cursors, filters and bits zeroed, its row table
// uploaded through `stage`.  *rows_dev stays null when the call has no bucket class.
static int upload_bucket_rows(dd_ctx* c, StageSet& stage, const std::vector<dd::SweepClass>& classes, int ngenomes, int kmin, int kmax, uint8_t* regs_dev,
                              const dd::BucketRow** rows_dev) {
    const dd::BucketLayout lay = dd::bucket_layout(classes, c->p, ngenomes, kmin, kmax);
    if (!lay.total) return DD_OK;
    std::vector<dd::BucketRow> rtab((size_t)ngenomes * lay.K);
    int rc;
    if ((rc = c->buckets.reserve(lay.total))) return rc;
    if ((rc = stage.rows.reserve(lay.cursors - lay.table))) return rc;
    char* bb = static_cast<char*>(c->buckets.p);
    dd::bucket_rows(lay, bb, regs_dev, c->p, ngenomes, rtab.data());
    DD_HIP(hipMemsetAsync(bb + lay.zero_begin, 0, lay.zero_bytes, c->stream));
    if ((rc = upload(c, stage.rows, bb + lay.table, rtab.data(), sizeof(dd::BucketRow) * rtab.size(), 0))) return rc;
    *rows_dev = reinterpret_cast<const dd::BucketRow*>(bb + lay.table);
    return DD_OK;
}

// The rows of sketch(U_k) that a call compares its rows with (dd_kernels.h, saturation): max(kfirst, kSatMinK) .. last_k, built here on the
// call's stream where this context has not built them yet.  last_k = 0: the call has no saturation exit.
static int ensure_universe(dd_ctx* c, int kfirst, int last_k) {
    if (!last_k) return DD_OK;
    const size_t m = (size_t)1 << c->p;
    int rc;
    if ((rc = c->universe.reserve((size_t)(dd::kSatMaxK - dd::kSatMinK + 1) * m))) return rc;
    for (int k = std::max(kfirst, dd::kSatMinK); k <= last_k; ++k) {
        if (c->universe_built[k - dd::kSatMinK]) continue;
        dd::launch_universe(static_cast<uint8_t*>(c->universe.p) + (size_t)(k - dd::kSatMinK) * m, k, c->p, c->canonical, c->stream);
        DD_HIP(hipGetLastError());
        c->universe_built[k - dd::kSatMinK] = true;
    }
    return DD_OK;
}

static void launch_lds_class(dd_ctx* c, const dd::SweepClass& sc, const dd::SweepGenome* gt, const dd::SweepJob* jt, int ngenomes, int kmin, int sat_last_k, hipStream_t ks) {
    if (sc.kclass == dd::kBitmapClass) {
        dd::launch_bitmap(gt, jt, (int)sc.jobs.size(), sc.kfirst, sc.klast, c->canonical, ks);
        dd::launch_bitmap_finish(gt, ngenomes, sc.kfirst, sc.klast, kmin, c->p, ks);
    } else if (sc.kclass == dd::kBigmapClass) {
        dd::launch_bigmap(gt, jt, (int)sc.jobs.size(), c->canonical, ks);
        dd::launch_bigmap_finish(gt, ngenomes, sc.kfirst, sc.klast, kmin, c->p, c->canonical, ks);
    } else {
        dd::launch_sweep(gt, jt, (int)sc.jobs.size(), sc.kclass, sc.plan, static_cast<const uint8_t*>(c->universe.p), sat_last_k, ks);
    }
}

// K1.  The k classes are independent.  On a big call the HASHED classes are launched back to back (running them side by
// side was measured neutral to slightly slower: they compete for the same VALUs).  The small-k class of such a call (log2m
// <= 16, no bucket class) is bound by latency and dispatch, not by the VALUs -- most of its workgroups read their flags and
// return --, so it goes to ONE side lane and runs beside the first hashed class instead of in front of it; the lane is joined
// behind the last hashed class (profiles/k1_small_k_side.txt; DD_NO_SIDE_SMALLK keeps it on the caller's stream).  On a SMALL
// call (under 12 000 LDS jobs, DD_SIDE_JOBS) -- one batch of
// the ingestion pipeline, a single genome -- every LDS class is only a few rounds of workgroups long and ends
// with a tail of idle CUs: there the classes go to side streams so that one's tail overlaps another's body.
// At log2m >= 17 every bucket class is a pipeline of its own -- scatter(e), (sort(e),) replay(e), scatter(e+1) ... over its own
// rows -- so, when there are filtered epochs, every class of the call gets a side stream: the tails of one class's launches
// are filled by the others' work, and the small-k classes (their rows are not bucketed) run beside the pipelines.  (Starting
// the pipelines one first-epoch scatter apart, and streams of different priorities, were measured and lost:
// profiles/r03_bucket_path.txt, r04_bucket_path.txt.)  A call whose only epoch is the unfiltered first one (many small
// genomes: 64 x 5 Mbp at log2m 20) runs its bucket classes one after the other instead: its scatter (returning LDS atomics,
// 4-byte stores) and its replay (HBM reads at 5 TB/s) each have the chip to themselves then -- 24.4 -> 22.9 ms with round 4's
// kernels (profiles/r04_bucket_path.txt); calls with filtered epochs keep the side streams (26.8 against 24.9 ms without).
// The plan lists its LDS classes before its bucket classes (tests/test_plan.py), so pipelines on the caller's stream start
// behind the joins of the LDS classes.  *blocks: the workgroups launched.
static int launch_classes(dd_ctx* c, const dd_ctx::PlanEntry& plan, const dd::SweepGenome* gtab, const dd::BucketRow* rows, int ngenomes, int kmin, int kmax, int sat_last_k, int* blocks) {
    const int K = kmax - kmin + 1;
    size_t lds_jobs = 0, side_jobs = 12000;
    int lds_classes = 0, hashed_lds = 0, nbucket = 0, nepochs = 0, rc;
    bool small_k = false;
    for (const dd::SweepClass& sc : plan.classes) {
        if (sc.plan.mode != dd::kBucketMode) lds_jobs += sc.jobs.size(), ++lds_classes;
        else nepochs = sc.plan.nepochs, ++nbucket;
        if (sc.kclass == dd::kBitmapClass) small_k = true;
        else if (sc.kclass >= 0 && sc.plan.mode != dd::kBucketMode) ++hashed_lds;
    }
    // (both switches are read per call and are no part of the plan: the job tables are the same with and without them)
    if (const char* s = getenv("DD_SIDE_JOBS")) side_jobs = (size_t)strtoull(s, nullptr, 10);
    const bool side = lds_classes > 1 && lds_jobs < side_jobs, side_b = nepochs > 1;
    const bool side_k = !side && !side_b && !nbucket && small_k && hashed_lds && c->p <= 16 && !getenv("DD_NO_SIDE_SMALLK");
    const bool forks = side || side_b || side_k;
    if (forks && (rc = ensure_side_streams(c, side_b ? (int)plan.classes.size() : side_k ? 1 : lds_classes))) return rc;
    // (launches that run side by side are timed as ONE span on the caller's stream: per-launch spans would overlap; it is
    // closed on return, when every side stream has been joined into the caller's stream.  A call that forks its small-k
    // class alone has no per-launch spans for the classes on the caller's stream either: they lie inside the phase's span
    // and would be counted twice, profiles/sketch_device_split.txt, point 4)
    Span phase(c, DD_KERNEL_SWEEP, forks);
    if (forks) DD_HIP(hipEventRecord(c->side_go, c->stream));
    SideLanes lanes{c};
    for (size_t i = 0; i < plan.classes.size(); ++i) {
        const dd::SweepClass& sc = plan.classes[i];
        const dd::SweepJob* jobs = reinterpret_cast<const dd::SweepJob*>(static_cast<char*>(plan.jobtab.p) + plan.job_off[i]);
        const bool bucket = sc.plan.mode == dd::kBucketMode;
        const bool on_lane = side_b || (side && !bucket) || (side_k && sc.kclass == dd::kBitmapClass), timed = !on_lane && !side_k;
        rc = lanes.run(on_lane, [&](hipStream_t ks) {
            if (!bucket) {
                Span span(c, DD_KERNEL_SWEEP, timed);
                launch_lds_class(c, sc, gtab, jobs, ngenomes, kmin, sat_last_k, ks);
            }
            const dd::ScatterParams sp{rows, K, sc.plan.logg, sc.plan.cap_chunks, sc.plan.nb_log2};
            for (int e = 0; bucket && e < sc.plan.nepochs; ++e) {
                const size_t j0 = sc.epoch_begin[e], j1 = sc.epoch_begin[e + 1];
                if (j1 == j0) continue;
                Span span(c, DD_KERNEL_SWEEP, timed);
                dd::launch_scatter(gtab, jobs + j0, (int)(j1 - j0), sc.kclass, sc.plan, sp, ks, e == 0);
                dd::launch_replay(rows, ngenomes, K, sc.kfirst - kmin, sc.klast - sc.kfirst + 1, sc.plan, ks, e == 0);
            }
        }, !side_k);
        if (rc) break;
        *blocks += (int)sc.jobs.size();
    }
    // (the small-k lane of a big call is joined here, behind the hashed classes: the caller's union and the next call's memset of
    // the bitmaps and flags are both on the caller's stream.  Also after an error: nothing may be left running unordered.)
    const int jrc = lanes.join();
    if (rc || jrc) return rc ? rc : jrc;
    DD_HIP(hipGetLastError());
    return DD_OK;
}

extern "C" {

int dd_sketch_device(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int ngenomes,
                     int kmin, int kmax, uint8_t* regs_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (ngenomes < 0 || !regs_dev || (ngenomes && (!fasta_dev || !nbytes)))
        return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    uint64_t tokens_ub = 0;
    for (int g = 0; g < ngenomes; ++g) {
        if (nbytes[g] && !fasta_dev[g]) return fail(DD_EINVAL, "genome %d: null buffer", g);
        if (reinterpret_cast<uintptr_t>(fasta_dev[g]) & 15)
            return fail(DD_EINVAL, "genome %d: device buffer must be 16-byte aligned", g);
        tokens_ub += nbytes[g];
    }
    DeviceGuard guard(c->device);
    const size_t K = (size_t)(kmax - kmin + 1), m = (size_t)1 << c->p;
    DD_HIP(hipMemsetAsync(regs_dev, 0, (size_t)ngenomes * K * m, c->stream));
    if (!ngenomes) return DD_OK;

    dd::PlanKnobs knobs = dd::PlanKnobs::from_env();
    // (longer epochs = fewer launches and sharper filters per record: +4 % on 13 x 3 Gbp at log2m 20 with 48 GiB)
    if (!getenv("DD_BUCKET_GB")) knobs.bucket_budget = c->bucket_budget;
    std::vector<dd::PackGenome> ptab;  // token streams of all genomes + one K0 scratch
    size_t max_chunks = 0;
    Bitmaps bm;
    int rc;
    if ((rc = layout_tokens(c, fasta_dev, nbytes, ngenomes, ptab, max_chunks))) return rc;
    const int sat_last_k = dd::plan_saturate_last_k(c->p, c->canonical, kmin, kmax, knobs, nbytes, ngenomes);
    if ((rc = reserve_bitmaps(c, knobs, nbytes, ngenomes, kmin, kmax, sat_last_k ? (size_t)ngenomes * K : 0, bm))) return rc;
    if ((rc = ensure_universe(c, kmin, sat_last_k))) return rc;
    std::vector<dd::SweepGenome> gtab(ngenomes);
    for (int g = 0; g < ngenomes; ++g) {
        const dd::TokenStream& ts = ptab[g].out;
        gtab[g] = dd::SweepGenome{ts.codes, ts.bad, ts.ntok, regs_dev + (size_t)g * K * m,
                                  bm.small ? bm.small + (size_t)g * dd::kBitmapStride : nullptr,
                                  bm.big ? bm.big + (size_t)g * bm.big_stride : nullptr,
                                  bm.sat ? bm.sat + (size_t)g * K : nullptr};
    }

    // genome tables up, K0 launched: the K1 job tables are planned on the host meanwhile
    const size_t pack_off = align_up(sizeof(dd::SweepGenome) * ngenomes, 256);
    const size_t gtab_bytes = pack_off + align_up(sizeof(dd::PackGenome) * ngenomes, 256);
    if ((rc = c->tables.reserve(gtab_bytes))) return rc;
    // this call's staging set may still be feeding the uploads of the call before last
    StageSet& stage = c->stage[c->stage_cur ^= 1];
    DD_HIP(hipEventSynchronize(stage.free));
    if ((rc = stage.tables.reserve(gtab_bytes))) return rc;
    char* tdev = static_cast<char*>(c->tables.p);
    if ((rc = upload(c, stage.tables, tdev, gtab.data(), sizeof(dd::SweepGenome) * ngenomes, 0))) return rc;
    if ((rc = upload(c, stage.tables, tdev + pack_off, ptab.data(), sizeof(dd::PackGenome) * ngenomes, pack_off))) return rc;
    {
        Span sp(c, DD_KERNEL_PACK);  // K0: pack every genome of the batch (three launches)
        dd::launch_pack_batch(reinterpret_cast<const dd::PackGenome*>(tdev + pack_off), ngenomes, max_chunks, c->stream);
    }
    DD_HIP(hipGetLastError());

    dd_ctx::PlanEntry* plan = nullptr;
    const dd::BucketRow* rows_dev = nullptr;
    int blocks = 0;
    if ((rc = cached_plan(c, stage, knobs, nbytes, ngenomes, kmin, kmax, &plan))) return rc;
    if ((rc = upload_bucket_rows(c, stage, plan->classes, ngenomes, kmin, kmax, regs_dev, &rows_dev))) return rc;
    DD_HIP(hipEventRecord(stage.free, c->stream));
    if ((rc = launch_classes(c, *plan, reinterpret_cast<const dd::SweepGenome*>(tdev), rows_dev, ngenomes, kmin, kmax, sat_last_k, &blocks))) return rc;
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
    dd::FileBuf fq;
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

}  // extern "C"
