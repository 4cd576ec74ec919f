// dd_k2_api.hip -- the entry points of the C ABI (include/dandd_hip.h) that work on register slabs: union, card / hist and
// the HLL schedules (progressive, pairwise, leave-out, subsets, extend, greedy).  Host-side orchestration only; the
// kernels are in dd_union, dd_pscan, dd_gram, dd_leaveout, dd_subsets and dd_extend.hip.
#include "dd_ctx.h"

namespace {

// the host form of a call: its slab of n x K rows of m registers into c->regs (with `extra` bytes of room behind it)
int leaves_to_regs(dd_ctx* c, const uint8_t* leaf, int n, int K, size_t extra = 0) {
    DeviceGuard guard(c->device);
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes + extra))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, leaf, bytes, hipMemcpyHostToDevice, c->stream));
    return DD_OK;
}
const uint8_t* regs_of(dd_ctx* c) { return static_cast<const uint8_t*>(c->regs.p); }

// histograms of njobs register rows into c->hist
int hist_rows(dd_ctx* c, const uint8_t* regs_dev, int njobs) {
    int rc;
    if ((rc = c->hist.reserve((size_t)njobs * 64 * sizeof(uint32_t)))) return rc;
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_hist(regs_dev, njobs, c->p, static_cast<uint32_t*>(c->hist.p), c->stream);
    }
    DD_HIP(hipGetLastError());
    return DD_OK;
}

// the smallest and largest register of each of the K columns: 2 K words through the head of c->gram (reserved by the
// caller) back to the host, where they decide tile sizes and plans
int register_range(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, std::vector<uint32_t>& rng) {
    rng.resize((size_t)K * 2);
    dd::launch_register_range(leaf_dev, n, K, c->p, static_cast<uint32_t*>(c->gram.p), c->stream);
    DD_HIP(hipMemcpyAsync(rng.data(), c->gram.p, rng.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- union
int dd_union_device(dd_ctx* c, const uint8_t* const* in_dev, int n, size_t len, uint8_t* out_dev) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || !in_dev || !out_dev) return fail(DD_EINVAL, "bad argument");
    if (len % 16) return fail(DD_EINVAL, "len must be a multiple of 16");
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = stage_table(c, c->ptrs, in_dev, sizeof(void*) * n))) return rc;
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
    if ((rc = hist_rows(c, regs_dev, njobs))) return rc;
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
    if ((rc = hist_rows(c, regs_dev, njobs))) return rc;
    return estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), (size_t)njobs, est);
}

int dd_card_batch(dd_ctx* c, const uint8_t* regs, int njobs, double* est) {
    if (check_ctx(c)) return DD_EINVAL;
    if (njobs < 0 || (njobs && (!regs || !est))) return fail(DD_EINVAL, "bad argument");
    if (!njobs) return DD_OK;
    int rc;
    if ((rc = leaves_to_regs(c, regs, njobs, 1))) return rc;
    return dd_card_batch_device(c, regs_of(c), njobs, est);
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
    if ((rc = stage_table(c, c->ord, orderings, sizeof(int32_t) * norder * n))) return rc;
    {
        Span sp(c, DD_KERNEL_UNION);
        // bit-plane AND-scan (dd_pscan.hip) where it applies; DD_PROGRESSIVE_STREAM=1 keeps the streaming kernel of
        // dd_union.hip (one LDS atomic per register per prefix) for A/B runs and for the equality test
        bool done = false;
        if (dd::pscan_usable(n, norder, c->p) && !getenv("DD_PROGRESSIVE_STREAM")) {
            if ((rc = c->gram.reserve(dd::pscan_scratch_bytes(n, K, c->p, norder)))) return rc;
            std::vector<uint32_t> rng;   // (which thresholds exist decides the tile size: 296 bytes back to the host)
            if ((rc = register_range(c, leaf_dev, n, K, rng))) return rc;
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
    int rc;
    if ((rc = leaves_to_regs(c, leaf, n, K))) return rc;
    return dd_progressive_device(c, regs_of(c), n, K, orderings, norder, card);
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
    if ((rc = estimates_from_hist(c, static_cast<const uint32_t*>(c->hist.p), njobs, tmp.data()))) return rc;
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
    int rc;
    if ((rc = leaves_to_regs(c, leaf, n, K))) return rc;
    return dd_pairwise_device(c, regs_of(c), n, K, card);
}

// -------------------------------------------------------------------------- leave-out
int dd_leave_out_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, const int32_t* group, int ngroups, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf_dev || !group || !card) return fail(DD_EINVAL, "bad argument");
    if (check_groups(group, ngroups, n)) return DD_EINVAL;
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
    if ((rc = stage_table(c, c->ord, tab.data(), sizeof(int32_t) * tab.size()))) return rc;
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
    int rc;
    if ((rc = leaves_to_regs(c, leaf, n, K))) return rc;
    return dd_leave_out_device(c, regs_of(c), n, K, group, ngroups, card);
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
    std::vector<uint32_t> rng;
    if ((rc = register_range(c, leaf_dev, n, K, rng))) return rc;
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
    if ((rc = stage_table(c, c->ord, tab.data(), sizeof(int32_t) * tab.size()))) return rc;
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
    int rc;
    if ((rc = leaves_to_regs(c, leaf, n, K))) return rc;
    return dd_subsets_device(c, regs_of(c), n, K, card);
}

// ---------------------------------------------------------------------- extend / greedy
namespace {

// one dd_extend step: cards of base U leaf[rows[r]] (base_dev null: of the rows themselves) -> card[nrows][K] on the host
int extend_step(dd_ctx* c, const uint8_t* base_dev, const uint8_t* leaf_dev, int K, const int32_t* rows, int nrows, double* card) {
    const size_t njobs = (size_t)nrows * K;
    int rc;
    if ((rc = c->hist.reserve((njobs + K) * 64 * sizeof(uint32_t)))) return rc;
    if ((rc = stage_table(c, c->ord, rows, sizeof(int32_t) * nrows))) return rc;
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
    if (check_greedy_walk(n, mode, cand, ncand, nfixed, nsteps)) return DD_EINVAL;
    return DD_OK;
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
    if ((rc = leaves_to_regs(c, leaf, n, K, base ? one : 0))) return rc;
    uint8_t* dev = static_cast<uint8_t*>(c->regs.p);
    if (base) DD_HIP(hipMemcpyAsync(dev + bytes, base, one, hipMemcpyHostToDevice, c->stream));   // the base row, behind the slab
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
        const int pick = greedy_pick(cards.data(), nrows, K, kmin, mode);
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
    if ((rc = leaves_to_regs(c, leaf, n, K))) return rc;
    return dd_greedy_device(c, regs_of(c), n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card);
}

}  // extern "C"
