// dd_k2_api.hip -- the entry points of the C ABI (include/dandd_hip.h) that work on register slabs: union, card / hist and
// the HLL schedules (progressive, pairwise, cross, leave-out, subsets, extend, greedy).  Host-side orchestration only; the
// kernels are in dd_union, dd_pscan, dd_gram, dd_leaveout, dd_subsets and dd_extend.hip.
//
// Every schedule has ONE body.  It takes its slab as a Slab (the slab frame): the two extern "C" forms of an entry, at the
// end of the file, only say where the slab is.  A body checks every rule of its entry, then asks slab_dev for the slab on
// the device, then runs its launches through hist_step (the histogram step).
#include "dd_ctx.h"

namespace {

// a call's slab of n x K rows of m registers: in host memory (the plain entries) or in HBM already (the _device entries)
struct Slab { const uint8_t* p; bool host; };

// ... on the device: where it is, or in c->regs (with `extra` bytes of room behind it) once the rules have passed
int slab_dev(dd_ctx* c, Slab s, int n, int K, const uint8_t*& dev, size_t extra = 0) {
    dev = s.p;
    if (!s.host) return DD_OK;
    const size_t bytes = ((size_t)n * K) << c->p;
    int rc;
    if ((rc = c->regs.reserve(bytes + extra))) return rc;
    DD_HIP(hipMemcpyAsync(c->regs.p, s.p, bytes, hipMemcpyHostToDevice, c->stream));
    dev = static_cast<const uint8_t*>(c->regs.p);
    return DD_OK;
}

// The histogram step: room for njobs histograms in c->hist, the entry's table of nwords (null: none, or staged by the
// entry) into c->ord, launch(hist, table) inside ONE DD_KERNEL_UNION span, the launch check, and the njobs estimates to
// the host (est null: the histograms stay in c->hist).  What `launch` reserves or reads back is inside the span; a code
// other than DD_OK from it ends the step.
template <class Launch>
int hist_step(dd_ctx* c, size_t njobs, const int32_t* table, size_t nwords, double* est, Launch launch) {
    int rc;
    if ((rc = c->hist.reserve(njobs * 64 * sizeof(uint32_t)))) return rc;
    if (table && (rc = stage_table(c, c->ord, table, sizeof(int32_t) * nwords))) return rc;
    uint32_t* hist = static_cast<uint32_t*>(c->hist.p);
    {
        Span sp(c, DD_KERNEL_UNION);
        if ((rc = launch(hist, static_cast<const int32_t*>(c->ord.p)))) return rc;
    }
    DD_HIP(hipGetLastError());
    return est ? estimates_from_hist(c, hist, njobs, est) : DD_OK;
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

// ------------------------------------------------------------------------------- union
// n rows of len bytes, given by address: host rows go behind one another into c->regs, the result behind them
int union_rows(dd_ctx* c, const uint8_t* const* in, bool host, int n, size_t len, uint8_t* out) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || !in || !out) return fail(DD_EINVAL, "bad argument");
    if (len % 16) return fail(DD_EINVAL, "len must be a multiple of 16");
    DeviceGuard guard(c->device);
    int rc;
    std::vector<const uint8_t*> ptrs;
    uint8_t* out_dev = out;
    if (host) {
        if ((rc = c->regs.reserve((size_t)(n + 1) * len))) return rc;
        uint8_t* base = static_cast<uint8_t*>(c->regs.p);
        for (int i = 0; i < n; ++i) {
            DD_HIP(hipMemcpyAsync(base + (size_t)i * len, in[i], len, hipMemcpyHostToDevice, c->stream));
            ptrs.push_back(base + (size_t)i * len);
        }
        in = ptrs.data(), out_dev = base + (size_t)n * len;
    }
    if ((rc = stage_table(c, c->ptrs, in, sizeof(void*) * n))) return rc;
    {
        Span sp(c, DD_KERNEL_UNION);
        dd::launch_union(static_cast<const uint8_t* const*>(c->ptrs.p), n, len, out_dev, c->stream);
    }
    DD_HIP(hipGetLastError());
    if (!host) return DD_OK;
    DD_HIP(hipMemcpyAsync(out, out_dev, len, hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// -------------------------------------------------------------------------------- card
// njobs rows: their estimates to `est`, or (est null) their histograms to `hist`
int card_rows(dd_ctx* c, Slab regs, int njobs, double* est, uint32_t* hist) {
    if (check_ctx(c)) return DD_EINVAL;
    if (njobs < 0 || (njobs && (!regs.p || (!est && !hist)))) return fail(DD_EINVAL, "bad argument");
    if (!njobs) return DD_OK;
    DeviceGuard guard(c->device);
    const uint8_t* regs_dev;
    int rc;
    if ((rc = slab_dev(c, regs, njobs, 1, regs_dev))) return rc;
    rc = hist_step(c, (size_t)njobs, nullptr, 0, est, [&](uint32_t* h, const int32_t*) {
        dd::launch_hist(regs_dev, njobs, c->p, h, c->stream);
        return DD_OK;
    });
    if (rc || est) return rc;
    DD_HIP(hipMemcpyAsync(hist, c->hist.p, (size_t)njobs * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    DD_HIP(hipStreamSynchronize(c->stream));
    return DD_OK;
}

// ------------------------------------------------------------------------- progressive
int progressive(dd_ctx* c, Slab leaf, int n, int K, const int32_t* orderings, int norder, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || norder < 1 || !leaf.p || !orderings || !card) return fail(DD_EINVAL, "bad argument");
    for (size_t i = 0; i < (size_t)norder * n; ++i)
        if (orderings[i] < 0 || orderings[i] >= n) return fail(DD_EINVAL, "ordering entry %d outside 0..%d", orderings[i], n - 1);
    DeviceGuard guard(c->device);
    const uint8_t* leaf_dev;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev))) return rc;
    return hist_step(c, (size_t)norder * n * K, orderings, (size_t)norder * n, card, [&](uint32_t* hist, const int32_t* ord) {
        // bit-plane AND-scan (dd_pscan.hip) where it applies; DD_PROGRESSIVE_STREAM=1 keeps the streaming kernel of
        // dd_union.hip (one LDS atomic per register per prefix) for A/B runs and for the equality test
        bool done = false;
        if (dd::pscan_usable(n, norder, c->p) && !getenv("DD_PROGRESSIVE_STREAM")) {
            int rc;
            if ((rc = c->gram.reserve(dd::pscan_scratch_bytes(n, K, c->p, norder)))) return rc;
            std::vector<uint32_t> rng;   // (which thresholds exist decides the tile size: 296 bytes back to the host)
            if ((rc = register_range(c, leaf_dev, n, K, rng))) return rc;
            done = dd::launch_progressive_pscan(leaf_dev, n, K, c->p, ord, norder, rng.data(), c->gram.p, hist, c->stream);
        }
        c->k2_path = done ? DD_K2_PROGRESSIVE_PSCAN : DD_K2_PROGRESSIVE_STREAM;
        if (!done) dd::launch_progressive(leaf_dev, n, K, c->p, ord, norder, hist, c->stream);
        return DD_OK;
    });
}

// ---------------------------------------------------------------------------- pairwise
int pairwise(dd_ctx* c, Slab leaf, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf.p || !card) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const uint8_t* leaf_dev;
    const size_t njobs = (size_t)n * n * K;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev))) return rc;
    // all pairs as int8 Gram matrices on the matrix cores (dd_gram.hip); DD_PAIRWISE_STREAM=1 keeps the streaming
    // kernel of dd_union.hip (one LDS atomic per register per pair) for A/B runs and for the equality test
    const bool gram = dd::gram_usable(n, c->p) && !getenv("DD_PAIRWISE_STREAM");
    if (gram && (rc = c->gram.reserve(dd::gram_scratch_bytes(n, K, c->p, nullptr)))) return rc;
    c->k2_path = gram ? DD_K2_PAIRWISE_GRAM : DD_K2_PAIRWISE_STREAM;
    c->k2_launches = 0;
    std::vector<double> tmp(njobs);
    rc = hist_step(c, njobs, nullptr, 0, tmp.data(), [&](uint32_t* hist, const int32_t*) {
        if (gram) {
            DD_HIP(hipMemsetAsync(hist, 0, njobs * 64 * sizeof(uint32_t), c->stream));
            c->k2_launches = dd::launch_pairwise_gram(leaf_dev, n, K, c->p, hist, c->gram.p, c->stream);
        } else {
            dd::launch_pairwise(leaf_dev, n, K, c->p, hist, c->stream);
        }
        return DD_OK;
    });
    if (rc) return rc;
    // lower triangle histograms are all-zero: give them the mirrored estimate afterwards
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int a = i <= j ? i : j, b = i <= j ? j : i;
            memcpy(card + ((size_t)i * n + j) * K, tmp.data() + ((size_t)a * n + b) * K, sizeof(double) * K);
        }
    return DD_OK;
}

// ------------------------------------------------------------------------------- cross
// The rectangle: na rows of slab a against nb rows of slab b.  Each slab where it lies: a host slab a goes into c->regs, a host
// slab b behind it (or to the head when a is in HBM already); a resident slab is read in place.  The na nb K histograms are
// taken in rounds over a's 64-row blocks, as many blocks as DD_CROSS_HIST_MB (1024 when unset; read on every call) holds of
// 64 nb K histograms -- one block at the least.
int cross(dd_ctx* c, Slab a, int na, Slab b, int nb, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (na < 1 || nb < 1 || K < 1 || !a.p || !b.p || !card) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t abytes = ((size_t)na * K) << c->p, bbytes = ((size_t)nb * K) << c->p;
    const uint8_t *a_dev, *b_dev;
    int rc;
    if ((rc = slab_dev(c, a, na, K, a_dev, b.host ? bbytes : 0))) return rc;
    if (b.host && a.host) {
        uint8_t* behind = static_cast<uint8_t*>(c->regs.p) + abytes;
        DD_HIP(hipMemcpyAsync(behind, b.p, bbytes, hipMemcpyHostToDevice, c->stream));
        b_dev = behind;
    } else if ((rc = slab_dev(c, b, nb, K, b_dev))) {
        return rc;
    }
    // the Gram form on the matrix cores (dd_gram.hip); DD_CROSS_STREAM=1 keeps the streaming kernel of dd_union.hip for A/B
    // runs and for the equality test
    const bool gram = dd::cross_gram_usable(c->p) && !getenv("DD_CROSS_STREAM");
    c->k2_path = gram ? DD_K2_CROSS_GRAM : DD_K2_CROSS_STREAM;
    c->k2_launches = 0;
    const char* mb = getenv("DD_CROSS_HIST_MB");
    const size_t budget = (size_t)(mb && atol(mb) > 0 ? atol(mb) : 1024) << 20;
    const size_t per_block = (size_t)64 * nb * K * 64 * sizeof(uint32_t);
    const int rows = 64 * (int)std::min<size_t>(std::max<size_t>(budget / per_block, 1), ((size_t)na + 63) / 64);   // of a, per round
    if (gram) {   // (the first round is the largest in units, the last one may split its rows finer: room for either)
        const int last = na % rows ? na % rows : rows;
        if ((rc = c->gram.reserve(std::max(dd::cross_scratch_bytes(std::min(rows, na), nb, K, c->p, nullptr),
                                           dd::cross_scratch_bytes(last, nb, K, c->p, nullptr)))))
            return rc;
    }
    for (int s0 = 0; s0 < na; s0 += rows) {
        const int cnt = std::min(rows, na - s0);
        const uint8_t* a_round = a_dev + (((size_t)s0 * K) << c->p);
        rc = hist_step(c, (size_t)cnt * nb * K, nullptr, 0, card + (size_t)s0 * nb * K, [&](uint32_t* hist, const int32_t*) {
            if (!gram) {
                dd::launch_cross_stream(a_round, cnt, b_dev, nb, K, c->p, hist, c->stream);
                return DD_OK;
            }
            if (s0 == 0) dd::launch_cross_range(a_dev, na, b_dev, nb, K, c->p, static_cast<uint32_t*>(c->gram.p), c->stream);
            c->k2_launches += dd::launch_cross_gram(a_round, cnt, b_dev, nb, K, c->p, hist, c->gram.p, c->stream);
            return DD_OK;
        });
        if (rc) return rc;
    }
    return DD_OK;
}

// -------------------------------------------------------------------------- leave-out
int leave_out(dd_ctx* c, Slab leaf, int n, int K, const int32_t* group, int ngroups, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf.p || !group || !card) return fail(DD_EINVAL, "bad argument");
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
    const uint8_t* leaf_dev;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev))) return rc;
    return hist_step(c, (size_t)(ngroups + 1) * K, tab.data(), tab.size(), card, [&](uint32_t* hist, const int32_t* slots) {
        dd::launch_leaveout(leaf_dev, K, c->p, slots, n, ngroups, hist, c->stream);
        return DD_OK;
    });
}

// ------------------------------------------------------------------------ all subsets
// dd_subsets.hip: every subset's histogram from threshold bit planes.  Columns are taken Kc at a time so that the
// histograms (2^n Kc 64 u32) stay within 256 MiB and the partial counts within 512 MiB.
int subsets(dd_ctx* c, Slab leaf, int n, int K, double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || n > 16) return fail(DD_EINVAL, "n=%d outside 1..16: the unions of all 2^n subsets are computed", n);
    if (K < 1 || !leaf.p || !card) return fail(DD_EINVAL, "bad argument");
    DeviceGuard guard(c->device);
    const size_t nsub = (size_t)1 << n;
    const int Kc = (int)std::min<size_t>((size_t)K, std::max<size_t>(1, ((size_t)256 << 20) / (nsub * 64 * sizeof(uint32_t))));
    const size_t part_budget = (size_t)512 << 20;
    const uint8_t* leaf_dev;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev))) return rc;
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
    std::vector<double> est;
    for (size_t i = 0; i < plans.size(); ++i) {
        const int k0 = (int)i * Kc, kc = std::min(Kc, K - k0);
        est.resize(nsub * kc);
        rc = hist_step(c, nsub * kc, nullptr, 0, est.data(), [&](uint32_t* hist, const int32_t* staged) {
            dd::launch_subsets(leaf_dev, n, K, c->p, k0, kc, plans[i], staged + wg_off[i], reinterpret_cast<const uint32_t*>(staged),
                               static_cast<uint32_t*>(c->gram.p), hist, c->stream);
            return DD_OK;
        });
        if (rc) return rc;
        for (size_t s = 0; s < nsub; ++s) memcpy(card + s * K + k0, est.data() + s * kc, sizeof(double) * kc);
    }
    for (int kk = 0; kk < K; ++kk) card[kk] = 0.0;   // the empty set
    return DD_OK;
}

// ---------------------------------------------------------------------- extend / greedy
// one dd_extend step: cards of base U leaf[rows[r]] (base_dev null: of the rows themselves) -> card[nrows][K] on the host
int extend_step(dd_ctx* c, const uint8_t* base_dev, const uint8_t* leaf_dev, int K, const int32_t* rows, int nrows, double* card) {
    const size_t njobs = (size_t)nrows * K;
    int rc;
    if ((rc = c->hist.reserve((njobs + K) * 64 * sizeof(uint32_t)))) return rc;   // row nrows: the base's own histograms
    return hist_step(c, njobs, rows, nrows, card, [&](uint32_t* hist, const int32_t* rows_dev) {
        dd::launch_extend(base_dev, leaf_dev, K, c->p, rows_dev, nrows, hist, c->stream);
        return DD_OK;
    });
}

// `base` is where the slab is: a host row goes behind the slab in c->regs; one in HBM is read in place, 16 bytes at a time
int extend(dd_ctx* c, const uint8_t* base, Slab leaf, int n, int K, const int32_t* rows, int nrows, double* card) {
    if (!rows) nrows = n;
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf.p || !card) return fail(DD_EINVAL, "bad argument");
    if (nrows < 1) return fail(DD_EINVAL, "nrows=%d: at least one row is needed", nrows);
    if (rows)
        for (int r = 0; r < nrows; ++r)
            if (rows[r] < 0 || rows[r] >= n) return fail(DD_EINVAL, "rows[%d]=%d outside 0..%d", r, rows[r], n - 1);
    if (!leaf.host && (uintptr_t)base % 16) return fail(DD_EINVAL, "base must be 16-byte aligned");
    std::vector<int32_t> all;
    if (!rows) {
        all.resize(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        rows = all.data();
    }
    DeviceGuard guard(c->device);
    const size_t one = (size_t)K << c->p;
    const uint8_t* leaf_dev;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev, base ? one : 0))) return rc;
    if (leaf.host && base) {
        uint8_t* behind = static_cast<uint8_t*>(c->regs.p) + one * n;
        DD_HIP(hipMemcpyAsync(behind, base, one, hipMemcpyHostToDevice, c->stream));
        base = behind;
    }
    return extend_step(c, base, leaf_dev, K, rows, nrows, card);
}

int greedy(dd_ctx* c, Slab leaf, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps, int32_t* order,
           double* card) {
    if (check_ctx(c)) return DD_EINVAL;
    if (n < 1 || K < 1 || !leaf.p || !cand || !order || !card) return fail(DD_EINVAL, "bad argument");
    if (kmin < 1 || kmin + K - 1 > 64) return fail(DD_EINVAL, "k window %d..%d outside 1..64", kmin, kmin + K - 1);
    if (check_greedy_walk(n, mode, cand, ncand, nfixed, nsteps)) return DD_EINVAL;
    DeviceGuard guard(c->device);
    const size_t one = (size_t)K << c->p;
    const uint8_t* leaf_dev;
    int rc;
    if ((rc = slab_dev(c, leaf, n, K, leaf_dev))) return rc;
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

}  // namespace

extern "C" {

// The two forms of an entry: the slab (dd_union: the rows and the result) in host memory, and `_device`: in HBM.
int dd_union(dd_ctx* c, const uint8_t* const* in, int n, size_t len, uint8_t* out) { return union_rows(c, in, true, n, len, out); }
int dd_union_device(dd_ctx* c, const uint8_t* const* in_dev, int n, size_t len, uint8_t* out_dev) {
    return union_rows(c, in_dev, false, n, len, out_dev);
}

double dd_ertl_mle(const uint32_t hist[64], int log2m) {
    return dd::ertl_mle(hist, log2m, dd::mle_relerr(log2m));
}
int dd_hist_batch_device(dd_ctx* c, const uint8_t* regs_dev, int njobs, uint32_t* hist) {
    return card_rows(c, {regs_dev, false}, njobs, nullptr, hist);
}
int dd_card_batch(dd_ctx* c, const uint8_t* regs, int njobs, double* est) { return card_rows(c, {regs, true}, njobs, est, nullptr); }
int dd_card_batch_device(dd_ctx* c, const uint8_t* regs_dev, int njobs, double* est) {
    return card_rows(c, {regs_dev, false}, njobs, est, nullptr);
}
int dd_card(dd_ctx* c, const uint8_t* regs, double* est) { return dd_card_batch(c, regs, 1, est); }

int dd_progressive(dd_ctx* c, const uint8_t* leaf, int n, int K, const int32_t* orderings, int norder, double* card) {
    return progressive(c, {leaf, true}, n, K, orderings, norder, card);
}
int dd_progressive_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, const int32_t* orderings, int norder, double* card) {
    return progressive(c, {leaf_dev, false}, n, K, orderings, norder, card);
}
int dd_pairwise(dd_ctx* c, const uint8_t* leaf, int n, int K, double* card) { return pairwise(c, {leaf, true}, n, K, card); }
int dd_pairwise_device(dd_ctx* c, const uint8_t* dev, int n, int K, double* card) { return pairwise(c, {dev, false}, n, K, card); }
int dd_cross(dd_ctx* c, const uint8_t* a, int na, const uint8_t* b, int nb, int K, double* card) {
    return cross(c, {a, true}, na, {b, true}, nb, K, card);
}
int dd_cross_device(dd_ctx* c, const uint8_t* a_dev, int na, const uint8_t* b_dev, int nb, int K, double* card) {
    return cross(c, {a_dev, false}, na, {b_dev, false}, nb, K, card);
}
int dd_cross_host_device(dd_ctx* c, const uint8_t* a, int na, const uint8_t* b_dev, int nb, int K, double* card) {
    return cross(c, {a, true}, na, {b_dev, false}, nb, K, card);
}
int dd_leave_out(dd_ctx* c, const uint8_t* leaf, int n, int K, const int32_t* group, int ngroups, double* card) {
    return leave_out(c, {leaf, true}, n, K, group, ngroups, card);
}
int dd_leave_out_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, const int32_t* group, int ngroups, double* card) {
    return leave_out(c, {leaf_dev, false}, n, K, group, ngroups, card);
}
int dd_subsets(dd_ctx* c, const uint8_t* leaf, int n, int K, double* card) { return subsets(c, {leaf, true}, n, K, card); }
int dd_subsets_device(dd_ctx* c, const uint8_t* dev, int n, int K, double* card) { return subsets(c, {dev, false}, n, K, card); }
int dd_extend(dd_ctx* c, const uint8_t* base, const uint8_t* leaf, int n, int K, const int32_t* rows, int nrows, double* card) {
    return extend(c, base, {leaf, true}, n, K, rows, nrows, card);
}
int dd_extend_device(dd_ctx* c, const uint8_t* base_dev, const uint8_t* leaf_dev, int n, int K, const int32_t* rows, int nrows,
                     double* card) {
    return extend(c, base_dev, {leaf_dev, false}, n, K, rows, nrows, card);
}
int dd_greedy(dd_ctx* c, const uint8_t* leaf, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed, int nsteps,
              int32_t* order, double* card) {
    return greedy(c, {leaf, true}, n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card);
}
int dd_greedy_device(dd_ctx* c, const uint8_t* leaf_dev, int n, int K, int kmin, int mode, const int32_t* cand, int ncand, int nfixed,
                     int nsteps, int32_t* order, double* card) {
    return greedy(c, {leaf_dev, false}, n, K, kmin, mode, cand, ncand, nfixed, nsteps, order, card);
}

}  // extern "C"
