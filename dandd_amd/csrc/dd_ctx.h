// dd_ctx.h -- the context behind the C ABI's opaque dd_ctx, and the host-side helpers the ABI's sources share
// (dd_api.hip: context, timing and stats, synth, dd_plan_sweep; dd_sketch_api.hip: sketch; dd_k2_api.hip: union, card and the
// HLL schedules, one body each over its slab frame -- Slab, slab_dev -- and its histogram step, hist_step;
// dd_exact_api.hip: exact count, schedules and greedy; dd_exact_emit_api.hip: the selected k-mers, where they lie and the pattern table;
// dd_exact_samples_api.hip: samples that are no inputs screened, painted, called, counted and laid along the genomes; all
// over dd_exact_host.h / dd_exact_passes.hip: call frame, pass driver, emission; dd_ingest.hip: the file-ingestion pipeline; dd_comm.hip: RCCL).  Callers see dandd_hip.h only.
#pragma once
#include "../../include/dandd_hip.h"
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>
#include "dd_common.h"
#include "dd_io.h"
#include "dd_kernels.h"
#include "dd_plan.h"

// the calling thread's last error (dd_last_error); ONE object for the whole library (defined in dd_api.hip)
extern thread_local std::string g_err;
inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt), vsnprintf(buf, sizeof buf, fmt, ap), va_end(ap);
    g_err = buf;
    return code;
}
#define DD_HIP(expr)                                                                                                     \
    do {                                                                                                                 \
        hipError_t e_ = (expr);                                                                                          \
        if (e_ != hipSuccess) return fail(DD_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
// grow-only allocations: device memory (DevBuf) and pinned host staging (HostBuf)
template <bool Host>
struct GrowBuf {
    void* p = nullptr; size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return DD_OK;
        release();
        size_t want = n + n / 8 + 256;
        if ((Host ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) {
            p = nullptr;
            return fail(DD_ENOMEM, Host ? "hipHostMalloc(%zu) failed" : "hipMalloc(%zu) failed", want);
        }
        cap = want;
        return DD_OK;
    }
    void release() {
        if (p) (void)(Host ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
};
using DevBuf = GrowBuf<false>;
using HostBuf = GrowBuf<true>;
struct TimedSpan { hipEvent_t a, b; };

// One of the ingestion pipeline's two buffer sets (batch b uses set b & 1): FASTA bytes in, register slabs out, a pinned
// bounce buffer for the results, the device decoders' inputs and tables, and the set's three events.
struct PipeSet {
    DevBuf fasta, regs; HostBuf out;
    // BGZF files inflated on the device (dd_ginflate.hip; single-member files: dd_gunzip.hip): compressed bytes, block table and error count of a batch
    DevBuf gz, jobs, err; HostBuf jobs_host, err_host;
    // single-member gzip files inflated on the device: symbols, windows, the piece tables (RawFile[], starts, lens, offs,
    // chunk0, crcs) and their host copies
    DevBuf sym, win, raw; HostBuf raw_host, crc_host;
    // kseq's record rules over device-inflated texts (dd_fastq.hip): the batch's TextJob table, newline counts and positions
    DevBuf txt; HostBuf txt_host;
    hipEvent_t h2d = nullptr, done = nullptr, d2h = nullptr;
    void release() {
        for (DevBuf* b : {&fasta, &regs, &gz, &jobs, &err, &sym, &win, &raw, &txt}) b->release();
        for (HostBuf* b : {&out, &jobs_host, &err_host, &raw_host, &crc_host, &txt_host}) b->release();
        for (hipEvent_t* e : {&h2d, &done, &d2h})
            if (*e) (void)hipEventDestroy(*e), *e = nullptr;
    }
};

// The ingestion pipeline's state on a context (dd_sketch_files, dd_ingest.hip): pinned host buffers for the loader
// threads, a copy stream, two buffer sets, and what the device decoders' refusals have decided
struct IngestState {
    std::vector<dd::FileBuf*> file_pool;
    hipStream_t copy_stream_b = nullptr;  // device-inflated batches alternate between two: a launch of the inflate kernel is as long as ONE block takes, two in flight hide each other
    hipStream_t copy_stream = nullptr, out_stream = nullptr;  // H2D and D2H on streams of their own: an in-order stream would park batch b+1's upload behind batch b's results
    PipeSet pipe[2];
    bool no_gpu_inflate = false;   // this context inflates on the host (set for the retry of a call, for good after three)
    int inflate_refusals = 0;      // calls in which the device decoder refused a block
    bool inflate_retry = false;    // ... and the call that met it is run again
    bool inflate_retry_counts = false;   // ... and counts towards the three strikes (a size mismatch or a lack of device memory does not:
                                         //     the decoder did its work, the FILE -- damaged trailer, two members, text beyond 4 GiB -- is not for it)
    // dd_inflate_files: the text of every file of the running dd_sketch_files pass, as K0 is about to read it, goes here
    struct TextSink { uint8_t* const* out; const size_t* caps; size_t* lens; bool short_buffer; };
    TextSink* text_sink = nullptr;
    int calls = 0;                // dd_sketch_files calls; ms: the last one's wall, waiting for loaders, batches, bytes (as a double)
    double ms[4] = {0, 0, 0, 0};
    void release() {
        for (dd::FileBuf*& fb : file_pool) delete fb, fb = nullptr;
        for (PipeSet& s : pipe) s.release();
        for (hipStream_t* s : {&copy_stream, &copy_stream_b, &out_stream})
            if (*s) (void)hipStreamDestroy(*s), *s = nullptr;
    }
};

// Pinned staging for the tables of one sketch call -- genome/pack tables, K1 job tables (their size is only known once K0
// is launched, and growing a buffer frees it) and the bucket rows -- and the event signalled when the last upload from
// them completed.  A context has two and dd_sketch_device alternates, so that a call can be issued while the uploads of the
// call before it are still queued behind work of other streams (the ingestion pipeline issues batch b + 1 while batch b
// waits for its files to be copied or inflated).
struct StageSet { HostBuf tables, jobs, rows; hipEvent_t free = nullptr; };

struct dd_ctx {
    int device = 0, p = 14, canonical = 1;
    hipStream_t stream = nullptr;
    bool timing = false;
    std::vector<TimedSpan> spans[DD_KERNEL_COUNT];
    std::vector<hipEvent_t> pool;
    // workspaces
    DevBuf tokens, scratch, tables, fasta, regs, ptrs, hist, est, ord, bitmaps, bigmaps, exact, buckets, gram, synth;
    DevBuf masks;  // dd_exact_greedy: cursor and overflow word | gains [64][64] | the mask streams of every k of the call
    DevBuf emit;   // dd_exact_select_kmers, dd_exact_locate (exact_records): cursor (256 B) | lo | hi | mask, `cap` records each
    DevBuf hits;   // what the kernels behind the ordered records write: dd_exact_locate's hit bitmaps, off[njobs] words; the parts each
                   // entry of dd_exact_samples_api.hip declares (HitsCarve; the layout stands in the comment above the entry)
    DevBuf pat[2]; // dd_exact_patterns: the running table in mask order (masks | counts) and where the next merge puts it, in turns
    // saturation (dd_kernels.h): sketch(U_k) for k = kSatMinK..kSatMaxK at this context's log2m and strand mode, [k - kSatMinK][m];
    // a row is built by the first call that needs it, on that call's stream, and kept
    DevBuf universe;
    bool universe_built[dd::kSatMaxK - dd::kSatMinK + 1] = {};
    StageSet stage[2];
    int stage_cur = 0;  // the set of the running (or last) sketch call
    // the job tables of the last few sketch calls: a call over genomes of the same sizes and the same k range (a
    // pipeline sketching batches of a few recurring shapes, a benchmark loop) reuses them, on the host and in HBM
    struct PlanEntry {
        bool valid = false;
        int kmin = 0, kmax = 0;
        std::vector<size_t> sizes;
        dd::PlanKnobs knobs;
        std::vector<dd::SweepClass> classes;
        std::vector<size_t> job_off;
        DevBuf jobtab;
        unsigned long long last_use = 0;
    };
    PlanEntry plans[8];
    unsigned long long plan_clock = 0;
    IngestState ingest;  // dd_sketch_files
    hipStream_t side[8] = {};  // k classes of a small call run side by side
    hipEvent_t side_done[8] = {}, side_go = nullptr;
    // HBM the record streams of one log2m >= 17 call may take: a sixth of the device (48 GiB of 288), 16 GiB at least
    size_t bucket_budget = (size_t)16 << 30;
    // stats of the last sketch call
    uint64_t st_tokens = 0, st_updates = 0;
    int st_blocks = 0;
    int k2_path = 0;  // DD_K2_*: what the last progressive / pairwise call ran
    int k2_launches = 0;  // gram_kernel / cross_kernel launches of the last pairwise / cross call (0: a streaming form)
    // multi-GPU (dd_comm_*): this context's rank in an RCCL communicator, one context = one process = one GPU
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    unsigned long long comm_calls[2] = {0, 0};   // all-reduces, all-gathers issued
};
struct DeviceGuard {  // the context's device for the scope of a call
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// CPUs this process may really use: the affinity mask capped by the cgroup quota (a container that shows
// 256 logical CPUs behind a 16-CPU quota must not get 256 loader threads)
inline int usable_cpus() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max(1, CPU_COUNT(&set));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32];
        long period = 0;
        if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
            n = std::min(n, std::max(1, (int)(atol(quota) / period)));
        fclose(f);
    }
    return n;
}
inline int check_ctx(dd_ctx* c) { return c ? DD_OK : fail(DD_EINVAL, "null context"); }

inline hipEvent_t get_event(dd_ctx* c) {
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
inline int upload(dd_ctx* c, HostBuf& stage, void* dst_dev, const void* src, size_t bytes, size_t stage_off) {
    if (!bytes) return DD_OK;
    memcpy(static_cast<char*>(stage.p) + stage_off, src, bytes);
    DD_HIP(hipMemcpyAsync(dst_dev, static_cast<char*>(stage.p) + stage_off, bytes,
                          hipMemcpyHostToDevice, c->stream));
    return DD_OK;
}

// A host table into `dst` (grown to hold it) through the current staging set.  The staging buffer may not be rewritten while
// the upload before this one is in flight: `free` is waited for first and recorded behind the copy.  (dd_sketch_device
// alternates the two sets around its launches and keeps its own sequence.)
inline int stage_table(dd_ctx* c, DevBuf& dst, const void* src, size_t bytes) {
    StageSet& s = c->stage[c->stage_cur];
    int rc;
    if ((rc = dst.reserve(bytes))) return rc;
    DD_HIP(hipEventSynchronize(s.free));
    if ((rc = s.tables.reserve(bytes))) return rc;
    if ((rc = upload(c, s.tables, dst.p, src, bytes, 0))) return rc;
    DD_HIP(hipEventRecord(s.free, c->stream));
    return DD_OK;
}

// histograms already on the device -> estimates on the host (device MLE, bit-identical to the
// host MLE: same IEEE operations, no contraction; asserted by tests/test_gpu_parity.py)
inline int estimates_from_hist(dd_ctx* c, const uint32_t* hist_dev, size_t njobs, double* est_host) {
    int rc = c->est.reserve(njobs * sizeof(double));
    if (rc) return rc;
    dd::launch_mle(hist_dev, njobs, c->p, static_cast<double*>(c->est.p), c->stream);
    DD_HIP(hipGetLastError());
    DD_HIP(hipMemcpyAsync(est_host, c->est.p, njobs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// K0's workspace for the n inputs of a call: every input's token stream (codes | bad | ntok, each 256-byte aligned) in
// c->tokens and its pack scratch in c->scratch.  ptab[g] is what K0 reads; ptab[g].out is where its tokens will be.
inline int layout_tokens(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, std::vector<dd::PackGenome>& ptab,
                         size_t& max_chunks) {
    std::vector<size_t> off_codes(n), off_bad(n), off_ntok(n), off_scratch(n);
    size_t tot = 0, scratch_tot = 0;
    for (int g = 0; g < n; ++g) {
        off_codes[g] = tot;
        tot += align_up(dd::codes_words(nbytes[g]) * 4, 256);
        off_bad[g] = tot;
        tot += align_up(dd::bad_words(nbytes[g]) * 4, 256);
        off_ntok[g] = tot;
        tot += 256;
        off_scratch[g] = scratch_tot;
        scratch_tot += align_up(dd::pack_scratch_bytes(nbytes[g]), 256);
    }
    int rc;
    if ((rc = c->tokens.reserve(tot))) return rc;
    if ((rc = c->scratch.reserve(scratch_tot))) return rc;
    char* tb = static_cast<char*>(c->tokens.p);
    char* sb = static_cast<char*>(c->scratch.p);
    ptab.resize(n);
    max_chunks = 0;
    for (int g = 0; g < n; ++g) {
        dd::TokenStream ts{reinterpret_cast<uint32_t*>(tb + off_codes[g]), reinterpret_cast<uint32_t*>(tb + off_bad[g]),
                           reinterpret_cast<unsigned long long*>(tb + off_ntok[g])};
        ptab[g] = dd::PackGenome{fasta_dev[g], nbytes[g], dd::pack_chunks(nbytes[g]),
                                 reinterpret_cast<long long*>(sb + off_scratch[g]), ts};
        max_chunks = std::max(max_chunks, ptab[g].nchunks);
    }
    return DD_OK;
}

// the walk rules that the HLL and the exact greedy share: mode, cand[] over n rows, nfixed <= nsteps <= ncand
inline int check_greedy_walk(int n, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps) {
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

// the selection rule of include/dandd_hip.h (dd_greedy): the largest card / k of the window, a later k winning a tie
inline double window_delta(const double* card, int K, int kmin) {
    double best = 0.0;
    for (int kk = 0; kk < K; ++kk) {
        const double v = card[kk] / (double)(kmin + kk);
        if (best <= v) best = v;
    }
    return best;
}

// ... and between candidates: the row of cards[nrows][K] with the largest (DD_GREEDY_MAX) or smallest window delta, the
// first of equals
inline int greedy_pick(const double* cards, int nrows, int K, int kmin, int mode) {
    int pick = 0;
    double best = window_delta(cards, K, kmin);
    for (int r = 1; r < nrows; ++r) {
        const double d = window_delta(cards + (size_t)r * K, K, kmin);
        if (mode == DD_GREEDY_MAX ? d > best : d < best) best = d, pick = r;
    }
    return pick;
}

// the group[] / ngroups rules that the HLL and the exact leave-out share
inline int check_groups(const int32_t* group, int ngroups, int n) {
    if (ngroups < 1) return fail(DD_EINVAL, "ngroups=%d: at least one group is needed", ngroups);
    if (ngroups > n) return fail(DD_EINVAL, "ngroups=%d is more than the %d leaves", ngroups, n);
    for (int i = 0; i < n; ++i)
        if (group[i] < -1 || group[i] >= ngroups) return fail(DD_EINVAL, "group[%d]=%d outside -1..%d", i, group[i], ngroups - 1);
    return DD_OK;
}
