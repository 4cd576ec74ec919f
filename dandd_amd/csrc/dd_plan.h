// dd_plan.h -- the K1 job tables: which workgroup sketches which (genome, k-group, tile range), and where the record
// path's rows lie in HBM.  Pure host code, no HIP calls: dd_sketch_device (dd_sketch_api.hip) uploads the tables, tests
// inspect them through dd_plan_sweep (include/dandd_hip.h) and tests/native/sanitize_host.cpp without a GPU.
#pragma once
#include <stddef.h>

#include <vector>

#include "dd_kernels.h"

namespace dd {

constexpr int kBitmapClass = -1;  // SweepClass::kclass of the small-k presence-bitmap class
constexpr int kBigmapClass = -2;  // ... of the k = 10 (, 11) big-bitmap class of log2m >= 19 (dd_kernels.h)

struct SweepClass {
    int kclass;      // kBitmapClass, or the window class of sweep_kernel: 0 (k <= 16), 1 (<= 32), 3 (33..48), 2 (49..64)
    int kfirst, klast;
    SweepPlan plan;  // launch shape of the class (mode, LDS bytes, threads)
    std::vector<SweepJob> jobs;
    // bucket mode (plan.mode == kBucketMode): the jobs of epoch e are jobs[epoch_begin[e] .. epoch_begin[e+1]);
    // one scatter launch per (class, epoch), one replay launch per epoch over the rows of all classes
    std::vector<size_t> epoch_begin;
};

// What the environment may change about a plan (README.md lists every knob): capacities, and the switches the tests use to
// reach, on small inputs, the paths large inputs take (several epochs, a full record stream, the exact-set class).
struct PlanKnobs {
    size_t bucket_e0_tiles = 0;     // DD_BUCKET_E0: tiles in the first epoch; 0 = four tokens per register (4 m / 65536), at least 8
    size_t bucket_emax_tiles = 0;   // DD_BUCKET_EMAX: longest epoch; 0 = what the budget below allows, at most 256 tiles
    size_t bucket_cap_chunks = 0;   // DD_BUCKET_CAP: 1024-record chunks per row's stream; 0 = every token of the first epoch fits
    size_t bucket_budget = (size_t)16 << 30;  // DD_BUCKET_GB: HBM for the record areas of one call
    bool bigmap_any_size = false;   // DD_BIGMAP_ANY_SIZE (tests): the exact-set class whatever the genomes' sizes
    bool saturate_any_size = false; // DD_SATURATE_ANY_SIZE (tests): the saturation exit (plan_saturate_last_k) whatever the genomes' sizes
    bool no_saturate = false;       // DD_NO_SATURATE: no saturation exit at all
    static PlanKnobs from_env();
    bool operator==(const PlanKnobs& o) const {
        return bucket_e0_tiles == o.bucket_e0_tiles && bucket_emax_tiles == o.bucket_emax_tiles && bucket_cap_chunks == o.bucket_cap_chunks &&
               bucket_budget == o.bucket_budget && bigmap_any_size == o.bigmap_any_size &&
               saturate_any_size == o.saturate_any_size && no_saturate == o.no_saturate;
    }
};

// the ks of a call that go to the big-bitmap class (false: none)
// (`nbytes`: the call's genomes -- an exact set only pays when a genome has several times more tokens than the
// set can have members, because every index tile's workgroup hashes the whole set afterwards)
bool plan_bigmap_range(int log2m, int kmin, int kmax, const PlanKnobs& knobs, const size_t* nbytes, int ngenomes, int* ka, int* kb);
// The last k of a call whose rows are checked against sketch(U_k) (dd_kernels.h, saturation), 0: none.  The ks are those of
// the call's range in kSatMinK..kSatMaxK for which some genome has nbytes >= 8 |U_k|: below that a row is not expected to
// saturate (random text needs |U_k| (ln m + 0.58) tokens) and the compare at every merge would only cost.  |U_k| grows with
// k, so they are a prefix of the hashed ks: max(kmin, kSatMinK) .. the value returned.  log2m <= 16 only (registers in LDS).
int plan_saturate_last_k(int log2m, int canonical, int kmin, int kmax, const PlanKnobs& knobs, const size_t* nbytes, int ngenomes);
std::vector<SweepClass> plan_sweep(int log2m, int canonical, const size_t* nbytes, int ngenomes, int kmin,
                                   int kmax, const PlanKnobs& knobs);

// Where the record path (log2m >= 17) keeps what in its ONE allocation, as byte offsets from its start.  The regions lie
// in this order: the BucketRow table; one cursor per (genome, k) row, each in a 256-byte slot of its own (every block of a
// row is reserved by an atomic add on it, and neighbouring rows are written from other XCDs); then, for the bucketed rows
// only -- those whose k belongs to a class of plan.mode == kBucketMode --, the 4-bit filters of (m >> logg) / 2 bytes
// (16-aligned), the rho = 1 bits of the first epoch (m / 8 bytes: one bit per register instead of a record each,
// dd_scatter.hip, scatter_first_bin_kernel), fill (cap_chunks * 4 bytes) + seg (cap_chunks * 32 bytes, at seg_off) each
// 256-aligned, and the record areas of cap_chunks * 4096 bytes (1024 records per chunk).  Bucketed row (g, kk) is number
// g * per_genome + slot[kk] of its regions.  [zero_begin, zero_begin + zero_bytes) = cursors, filters and bits must start
// a call at zero: nothing handed out, every register's lower bound 0.  A wrong offset here does not crash: one row's
// records land in another row's stream and the registers come out slightly low (tests/native/sanitize_host.cpp).
struct BucketLayout {
    int K = 0, per_genome = 0;  // rows of a genome; how many of them are bucketed
    std::vector<int> slot;      // [K]: -1 = the row is not bucketed
    size_t table = 0, cursors = 0, filters = 0, ones = 0, fills = 0, areas = 0;                                 // region starts
    size_t cursor_stride = 256, filter_bytes = 0, ones_bytes = 0, fill_bytes = 0, seg_off = 0, area_bytes = 0;  // per row
    size_t zero_begin = 0, zero_bytes = 0, total = 0;  // (total 0: the call has no bucket class)
};
BucketLayout bucket_layout(const std::vector<SweepClass>& classes, int log2m, int ngenomes, int kmin, int kmax);
// the call's row table over an allocation at `base`, row (g, kk)'s registers at regs + (g * K + kk) * m
void bucket_rows(const BucketLayout& lay, char* base, uint8_t* regs, int log2m, int ngenomes, BucketRow* rows);

}  // namespace dd
