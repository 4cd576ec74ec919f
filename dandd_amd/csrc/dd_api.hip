// dd_api.hip -- the C ABI of libdandd_hip.so (declared in include/dandd_hip.h).
//
// Host-side orchestration only: workspace management in HBM, job tables for the sweep,
// stream/event plumbing.  Every entry point names the DandD command line it replaces in
// include/dandd_hip.h.  There is no CPU fallback anywhere in this file.  Here: context, timing and stats,
// synth, dd_plan_sweep.  The sketch is in dd_sketch_api.hip, union, card and the HLL schedules in dd_k2_api.hip,
// the exact count and schedules in dd_exact_api.hip, the file-ingestion pipeline (dd_sketch_fasta,
// dd_sketch_files, dd_inflate_files) in dd_ingest.hip, RCCL in dd_comm.hip; the helpers they share are in dd_ctx.h.
#include "dd_ctx.h"

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
    if (hipEventCreateWithFlags(&c->stage[0].free, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->stage[1].free, hipEventDisableTiming) != hipSuccess) {
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
    for (auto& pe : c->plans) pe.jobtab.release();
    for (DevBuf* b : {&c->tokens, &c->scratch, &c->tables, &c->fasta, &c->regs, &c->ptrs, &c->hist,
                      &c->est, &c->ord, &c->bitmaps, &c->bigmaps, &c->exact, &c->buckets, &c->gram, &c->synth, &c->masks, &c->emit, &c->hits, &c->pat[0], &c->pat[1], &c->universe})
        b->release();
    for (StageSet& s : c->stage) {
        if (s.free) (void)hipEventDestroy(s.free);
        for (HostBuf* b : {&s.tables, &s.jobs, &s.rows}) b->release();
    }
    c->ingest.release();
    for (int i = 0; i < 8; ++i)
        if (c->side[i]) {
            (void)hipStreamDestroy(c->side[i]);
            (void)hipEventDestroy(c->side_done[i]);
        }
    if (c->side_go) (void)hipEventDestroy(c->side_go);
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

int dd_last_k2_launches(dd_ctx* c) {
    if (check_ctx(c)) return DD_EINVAL;
    return c->k2_launches;
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

