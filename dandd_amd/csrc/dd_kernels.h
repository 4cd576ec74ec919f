// dd_kernels.h -- host-callable launchers of the gfx950 kernels behind the C ABI.
#pragma once
#include <atomic>
#include <type_traits>
#include <vector>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dd {

// ---- host: pick an instantiation, launch it ------------------------------------------------------------------------------
// f(std::bool_constant<b>)
template <typename F>
void dispatch_bool(bool b, const F& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// Launch of a kernel whose dynamic LDS may exceed 64 KiB: that must be allowed per kernel AND per device (a process may hold
// contexts on several GPUs), once, not on every launch; remembered in one bit per device id.  STATIC_LDS: the kernel's own
// __shared__ bytes -- dynamic + static must stay within the CU's 160 KiB or the call is refused.
template <auto Kern, int STATIC_LDS = 0, typename... Args>
void launch_full_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, Args... args) {
    static std::atomic<unsigned long long> allowed{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(allowed.load(std::memory_order_relaxed) & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - STATIC_LDS) != hipSuccess)
            (void)hipGetLastError();  // not sticky: a launch that needs the room will report it
        allowed.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, args...);
}

// ---------------------------------------------------------------------------------------
// Token stream of one genome in HBM (output of K0, input of K1).
//   codes : 2 bits per token, token j of word w at bits [2j, 2j+1]   (16 tokens / u32);
//           unspecified for BREAK tokens (no window that contains one is ever used)
//   bad   : 1 bit per token, 1 = BREAK (non-ACGT byte or record boundary) (32 tokens / u32)
//   ntok  : device scalar, number of tokens; the stream is padded with BREAKs to a
//           multiple of 64 tokens (one K1 thread segment).
// ---------------------------------------------------------------------------------------
struct TokenStream {
    uint32_t* codes;
    uint32_t* bad;
    unsigned long long* ntok;
};

constexpr int kPackThreads = 256;
constexpr int kPackBytesPerThread = 64;
constexpr int kPackChunk = kPackThreads * kPackBytesPerThread;  // 16 KiB of FASTA per K0 workgroup
constexpr int kSegTokens = 64;                 // tokens per K1 thread segment

// scratch for one K0 run over n bytes: 4 x int64 per chunk, + one for the position of the first header character
inline size_t pack_chunks(size_t n) { return (n + kPackChunk - 1) / kPackChunk; }
inline size_t pack_scratch_bytes(size_t n) { return ((pack_chunks(n) + 1) * 4 + 2) * sizeof(long long); }
// capacity (in u32 words) of the code / bad arrays for an n-byte FASTA (tokens <= n)
inline size_t codes_words(size_t n) { return ((n + 63) / 64 + 1) * 4; }
inline size_t bad_words(size_t n) { return ((n + 63) / 64 + 1) * 2; }

struct PackGenome {             // one per genome, device-resident table
    const uint8_t* fa;          // FASTA bytes, 16-byte aligned
    size_t n;                   // bytes
    size_t nchunks;             // pack_chunks(n)
    long long* scratch;         // pack_scratch_bytes(n)
    TokenStream out;
};
// gridDim.y = genome: every genome of the batch is packed by the same three launches
void launch_pack_batch(const PackGenome* tab_dev, int ngenomes, size_t max_chunks, hipStream_t st);

// ---------------------------------------------------------------------------------------
// K1: fused k-sweep sketch.
// ---------------------------------------------------------------------------------------
struct SweepGenome {            // one per genome, device-resident table
    const uint32_t* codes;
    const uint32_t* bad;
    const unsigned long long* ntok;
    uint8_t* regs;              // [K][m] for this genome
    uint32_t* bitmap;           // presence bitmaps of the canonical k-mers, k = 1..kBitmapMaxK (or null)
    uint32_t* bigmap;           // presence bitmaps of k = 10 (, 11) at log2m >= 19 (or null): bigmap_offset_words
    uint32_t* sat;              // one "saturated" flag per row of the genome's slab, zeroed per call (or null: no early exit in this call)
};

// Small-k path: for k <= kBitmapMaxK there are at most 4^k <= 262144 distinct k-mers, so K1 only
// records WHICH k-mers occur (one LDS bit each) and hashes every distinct one once afterwards.
constexpr int kBitmapMaxK = 9;           // (k = 10 was tried as a 128 KiB class of its own: its set completes too late to pay)
constexpr int kBitmapWords = 10924;      // sum over k = 1..9 of max(1, 4^k / 32)
constexpr int kBitmapStride = 11008;     // words per genome (256-byte multiple); the slack holds one "complete" flag per k
// first word of k's bitmap inside a genome's block
inline constexpr int bitmap_offset(int k) {
    int off = 0;
    for (int j = 1; j < k; ++j) off += (j < 3) ? 1 : (1 << (2 * j - 5));
    return off;
}
inline constexpr int bitmap_words(int k) { return (k < 3) ? 1 : (1 << (2 * k - 5)); }
// Second small-k class, bucket mode at log2m >= 19 only: k = 10 (and k = 11 at log2m 20).  There a row has fewer
// distinct k-mers than (about twice) its registers, a register group almost always holds an EMPTY register, the
// group-minimum filter lets everything through and every update pays a probe of the row: 2.4 ms per k against
// 1.0 for the other rows (10 x 50 Mbp).  The k-mer set itself is smaller than the row, so it is recorded
// exactly, in 128 KiB slices of LDS (one workgroup per CU), and each distinct k-mer is hashed afterwards.
// Index of a k-mer: the canonical value (2k bits); for odd k in canonical mode the strand whose MIDDLE base is
// A or C with that base's high bit dropped (2k - 1 bits: one of a k-mer and its reverse complement always
// qualifies), which halves the slices of k = 11.
constexpr int kBigmapMinK = 10, kBigmapMaxK = 11;
constexpr int kBigmapSliceWords = 1 << 15;  // 2^20 bits
inline constexpr int bigmap_last_k(int log2m) { return log2m >= 20 ? 11 : (log2m >= 19 ? 10 : 0); }
inline constexpr int bigmap_bits(int k, bool canon) { return (canon && (k & 1)) ? 2 * k - 1 : 2 * k; }
inline constexpr int bigmap_slices(int k, bool canon) { return 1 << (bigmap_bits(k, canon) - 20); }
inline constexpr size_t bigmap_offset_words(int k, bool canon) {  // k's first word in a genome's block
    size_t off = 0;
    for (int j = kBigmapMinK; j < k; ++j) off += (size_t)bigmap_slices(j, canon) * kBigmapSliceWords;
    return off;
}
struct SweepJob {               // one per workgroup, device-resident table
    int genome;
    int kfirst;                 // first k of the group (consecutive ks)
    int nk;                     // number of ks in the group (<= slots that fit LDS)
    int krow;                   // row of kfirst in the genome's [K][m] slab
    unsigned tile_begin, tile_end;  // tiles of (threads x 64) tokens
    int slice;                  // big-bitmap jobs: which 2^20-bit slice of k's index space the workgroup records
};
constexpr int kBucketMode = 5;
constexpr int kBucketFromLog2m = 17;  // registers stay in HBM (scatter + replay) from this log2m on
constexpr unsigned kRaiseQueueRecords = 128;                        // sweep_kernel's raise queue (dd_k1.h, RaiseQueue): records per wave
constexpr unsigned kRaiseQueueBytes = 16 * kRaiseQueueRecords * 4;  // ... bytes per 1024-thread workgroup
struct SweepPlan {
    int log2m;
    int canonical;
    int threads;                // workgroup size
    int lds_bytes;              // dynamic LDS per workgroup
    int queue_off = 0;          // mode 0, k classes 1 / 3 / 2: LDS byte offset of the raise queues behind the group's registers (dd_k1.h), 0 = none
    int mode;                   // 0: registers in LDS (log2m <= 16); 5 (kBucketMode): in HBM, scatter to buckets + replay (below)
    // kBucketMode only
    int logg = 0;               // one 4-bit filter entry (bounds saturate at 15, two entries per byte) per 2^logg registers
    int nb_log2 = 0;            // 2^nb_log2 index tiles of 64 KiB per row (replay)
    unsigned cap_chunks = 0;    // 1024-record chunks per row and epoch
    int nepochs = 0;
};
// Saturation (log2m <= 16, k = kSatMinK..kSatMaxK): the k-mer universe U_k is finite, registers are byte maxima, so a row can
// never pass sketch(U_k) -- the row all (canonical) k-mers hashed once give -- and a row that EQUALS it is final, long before
// the set of its k-mers is complete: only the one k-mer that holds each register's maximum has to have been seen (about
// |U_k| (ln m + 0.58) tokens of random text).  sweep_kernel compares at its merge, raises SweepGenome::sat of the row, and
// jobs that start later leave a flagged prefix of their group out.  universe: [k - kSatMinK][m], rows kSatMinK..universe_last_k
// built (launch_universe); universe_last_k = 0: no row is compared or skipped.
constexpr int kSatMinK = 10, kSatMaxK = 14;
// |U_k|: the k-mers there are, a k-mer and its reverse complement counted once in canonical mode (even k has palindromes)
inline constexpr size_t universe_size(int k, bool canon) {
    return canon ? ((size_t)1 << (2 * k - 1)) + ((k & 1) ? 0 : ((size_t)1 << (k - 1))) : (size_t)1 << (2 * k);
}
// row_dev[m] = sketch(U_k), zeroed here; log2m <= 16
void launch_universe(uint8_t* row_dev, int k, int log2m, int canonical, hipStream_t st);
void launch_sweep(const SweepGenome* genomes_dev, const SweepJob* jobs_dev, int njobs, int kclass,
                  const SweepPlan& plan, const uint8_t* universe_dev, int universe_last_k, hipStream_t st);

// ---------------------------------------------------------------------------------------
// K1 for log2m >= 17 (one register array does not fit LDS twice per CU, or at all; DandD's default is -r 20,
// /root/reference/lib/dandd_cmd.py:187): three kernels per EPOCH (a range of token tiles).
//   scatter: hash every k-mer of the epoch; an update whose rho cannot exceed the filter's lower bound
//            for its register group is dropped, the others are queued per wave in LDS, checked 64 at a time
//            against the row itself, and what survives leaves as 4-byte records (idx | rho << 24), one 256-byte
//            block at a time, for the ROW's record stream -- a dense stream: waves reserve 256 records per atomic
//            add on the row's cursor.  The first epoch (registers all zero) has no filter and no queues: a record goes
//            straight from the hash into the bin of its index tile (16 fixed regions of 4480 records per tile of tokens,
//            counts in seg[chunk][16]), except the updates of rho = 1 -- half of them --, which set a bit of BucketRow::ones.
//   sort   : every 1024-record chunk is sorted by index tile in place (HBM-bound streaming pass; not needed
//            after the first epoch).
//   replay : one workgroup per (row, 64 KiB index tile): tile into LDS, apply the tile's segment of every
//            chunk with LDS operations, store the tile back with plain 16-byte stores and refresh the
//            tile's filter.
// The filter of epoch e is exact knowledge of the registers after epoch e-1, so what scatter drops can
// never matter; the first epoch is four tokens per register long, each later one as long as all before it.
// ---------------------------------------------------------------------------------------
struct BucketRow {              // one per (genome, k) row of the call: table[genome * K + (k - kmin)]
    uint8_t* regs;              // the row's m registers in the caller's slab
    uint32_t* area;             // record stream: chunk c at area + c * 1024; null = row not bucketed
    uint32_t* cursor;           // records reserved this epoch, in blocks of 64 (may run past the capacity: overflow)
    uint32_t* fill;             // [cap_chunks] records of each chunk after the sort dropped the null ones
    uint16_t* seg;              // [cap_chunks][16] where each index tile's records start inside a sorted chunk
    uint8_t* filter;            // [m >> logg] lower bound per register group
    uint32_t* ones;             // [m / 32] first epoch: bit r = register r saw an update with rho = 1
};
struct ScatterParams {
    const BucketRow* rows;
    int K;                      // rows per genome
    int logg;
    unsigned cap_chunks;
    int nb_log2;                // index tiles per row (log2)
};
void launch_scatter(const SweepGenome* genomes_dev, const SweepJob* jobs_dev, int njobs, int kclass,
                    const SweepPlan& plan, const ScatterParams& sp, hipStream_t st, bool first_epoch);
// (sort +) replay + cursor reset of rows k0 .. k0+nks-1 (indices into a genome's K rows) of every genome; first_epoch: the
// records are the binned tiles the first epoch's scatter left (no sort pass)
void launch_replay(const BucketRow* rows_dev, int ngenomes, int K, int k0, int nks, const SweepPlan& plan, hipStream_t st, bool first_epoch);
int sweep_max_lds_bytes();
// small-k class: jobs carry ks <= kBitmapMaxK; records k-mer presence in genome.bitmap
// (kfirst..klast: the ks of the class; the LDS image covers exactly their bitmaps)
void launch_bitmap(const SweepGenome* genomes_dev, const SweepJob* jobs_dev, int njobs, int kfirst, int klast,
                   int canonical, hipStream_t st);
// one workgroup per (genome, k in [kfirst, klast]): hash every recorded k-mer once into slab row k-kmin
// big-bitmap class (log2m >= 19): jobs carry one k and one slice each; finish hashes the recorded sets into rows
// kfirst..klast, one workgroup per (k, genome, 64 KiB index tile)
void launch_bigmap(const SweepGenome* genomes_dev, const SweepJob* jobs_dev, int njobs, int canonical, hipStream_t st);
void launch_bigmap_finish(const SweepGenome* genomes_dev, int ngenomes, int kfirst, int klast, int kmin, int log2m,
                          int canonical, hipStream_t st);
void launch_bitmap_finish(const SweepGenome* genomes_dev, int ngenomes, int kfirst, int klast, int kmin,
                          int log2m, hipStream_t st);

// ---------------------------------------------------------------------------------------
// K2: byte-max union + 64-bin histograms.
// ---------------------------------------------------------------------------------------
void launch_union(const uint8_t* const* in_dev, int n, size_t len, uint8_t* out_dev, hipStream_t st);
void launch_hist(const uint8_t* regs_dev, int njobs, int log2m, uint32_t* hist_dev, hipStream_t st);
// running max along each ordering; hist[(o*n + j)*K + kk][64]
void launch_progressive(const uint8_t* leaf_dev, int n, int K, int log2m, const int32_t* ord_dev,
                        int norder, uint32_t* hist_dev, hipStream_t st);
// hist[((i*n)+j)*K + kk][64] for i <= j
void launch_pairwise(const uint8_t* leaf_dev, int n, int K, int log2m, uint32_t* hist_dev,
                     hipStream_t st);
// the same histograms through int8 Gram matrices on the matrix cores (dd_gram.hip); hist_dev zeroed by the caller
bool gram_usable(int n, int log2m);
size_t gram_scratch_bytes(int n, int K, int log2m, int* sp_per_launch);
int launch_pairwise_gram(const uint8_t* leaf_dev, int n, int K, int log2m, uint32_t* hist_dev, void* scratch,
                         hipStream_t st);   // (the gram_kernel launches it enqueued)
void launch_register_range(const uint8_t* leaf_dev, int n, int K, int log2m, uint32_t* rng_dev, hipStream_t st);
// the rectangle, na rows of slab a against nb rows of slab b: hist[((s*nb)+j)*K + kk][64] for every s < na, j < nb.  The
// streaming kernel (dd_union.hip) zeroes what it needs; the Gram form (dd_gram.hip, log2m >= 12) writes every word and wants
// the register ranges of BOTH slabs at the head of its scratch (launch_cross_range; a_dev may then be a part of the rows)
void launch_cross_stream(const uint8_t* a_dev, int na, const uint8_t* b_dev, int nb, int K, int log2m, uint32_t* hist_dev, hipStream_t st);
bool cross_gram_usable(int log2m);
size_t cross_scratch_bytes(int na, int nb, int K, int log2m, int* sp_per_launch);
void launch_cross_range(const uint8_t* a_dev, int na, const uint8_t* b_dev, int nb, int K, int log2m, uint32_t* rng_dev, hipStream_t st);
int launch_cross_gram(const uint8_t* a_dev, int na, const uint8_t* b_dev, int nb, int K, int log2m, uint32_t* hist_dev, void* scratch,
                      hipStream_t st);   // (the cross_kernel launches it enqueued)
// progressive unions as a bit-plane AND-scan (dd_pscan.hip); the streaming launch_progressive stays as the fallback
bool pscan_usable(int n, int norder, int log2m);
size_t pscan_scratch_bytes(int n, int K, int log2m, int norder);
bool launch_progressive_pscan(const uint8_t* leaf_dev, int n, int K, int log2m, const int32_t* ord_dev, int norder, const uint32_t* rng_host,
                              void* scratch, uint32_t* hist_dev, hipStream_t st);
void launch_mle(const uint32_t* hist_dev, size_t njobs, int log2m, double* est_dev, hipStream_t st);
// leave-out unions (dd_leaveout.hip): hist[g*K + kk][64] = |union of the leaves outside group g|, g < G; row G*K + kk the
// full union.  tab_dev[nslots][2]: (leaf row, group if the slot ends its group -- -1 the floor -- else -2), the leaves of a
// group consecutive, the floor first.  Zeroes hist_dev itself.
void launch_leaveout(const uint8_t* leaf_dev, int K, int log2m, const int32_t* tab_dev, int nslots, int G, uint32_t* hist_dev,
                     hipStream_t st);
// extend unions (dd_extend.hip): hist[(r*K + kk)][64] = histogram of the byte-max of base[kk] and leaf[rows[r]][kk], r < nrows; row
// nrows*K + kk: base's own.  base_dev null: the empty sketch (the rows' own histograms; row nrows stays zero).  base_dev 16-byte
// aligned.  Zeroes hist_dev ((nrows + 1) K 64 u32) itself.
void launch_extend(const uint8_t* base_dev, const uint8_t* leaf_dev, int K, int log2m, const int32_t* rows_dev, int nrows,
                   uint32_t* hist_dev, hipStream_t st);
// the empty base of launch_extend (dd_union.hip: hist_kernel over a row list): hist[(r * K + kk)][64] of leaf[rows[r]][kk] itself;
// hist_dev zeroed by the caller
void launch_rows_hist(const uint8_t* leaf_dev, int K, int log2m, const int32_t* rows_dev, int nrows, uint32_t* hist_dev, hipStream_t st);
// the end of both correction forms (dd_leaveout.hip): rows 0..nrows-1 of hist[.][K][64] hold corrections, add row nrows to them
void launch_corr_finish(uint32_t* hist_dev, int nrows, int K, hipStream_t st);
// base = byte-max(base, row) over len bytes (a multiple of 16)
void launch_extend_fold(uint8_t* base_dev, const uint8_t* row_dev, size_t len, hipStream_t st);
// all-subset unions (dd_subsets.hip) of columns k0 .. k0 + Kc - 1: hist[(s * Kc + kk)][64] = histogram of the byte-max over
// the leaves in mask s, s < 2^n (n <= 16); s = 0 gets m in bin 0.  rng as launch_register_range leaves it (all K columns).
// wg: (column, first job, threshold offset) per workgroup, uploaded by the caller; part: part_bytes of scratch.
struct SubsetsPlan {
    int HC = 1, nchunks = 1, RR = 1, D = 1, tiles = 1;
    size_t part_bytes = 0, lds_bytes = 0;
    std::vector<int32_t> wg;
};
SubsetsPlan plan_subsets(int n, int log2m, const uint32_t* rng_host, int k0, int Kc, size_t part_budget);
void launch_subsets(const uint8_t* leaf_dev, int n, int K, int log2m, int k0, int Kc, const SubsetsPlan& plan, const int32_t* wg_dev,
                    const uint32_t* rng_dev, uint32_t* part_dev, uint32_t* hist_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// exact distinct k-mer count (KMC stand-in): extract -> radix sort -> count distinct
// ---------------------------------------------------------------------------------------
struct ExactGenome {
    const uint32_t* codes;
    const uint32_t* bad;
    const unsigned long long* ntok;
    unsigned long long base;    // first slot of this genome in the k-mer arrays
};
// mode 0: every k-mer to its token's slot; counters[0] += valid k-mers written, counters[1] |= 1 if a valid
//         k-mer is all-ones (T^k, non-canonical)
// mode 1: hist[4096] += k-mers per bin of the k-mer space (kExactBins bins by a mix of the k-mer)
// mode 2: k-mers of bins [bin_lo, bin_hi) appended densely from slot counters[3] on (counters[3] += their number)
// tag (modes 0, 2): 1 = the genome's index in the key's top byte, 2 = in g[slot] (exact_tag_mode below); 0 = keys only
constexpr int kExactBins = 4096;
void launch_kmer_extract(const ExactGenome* tab_dev, int ng, size_t max_segments, int k, int canonical,
                         uint64_t* lo, uint64_t* hi, unsigned long long* counters, hipStream_t st, int mode = 0,
                         unsigned long long* hist = nullptr, uint32_t bin_lo = 0, uint32_t bin_hi = 0, int tag = 0,
                         uint8_t* g = nullptr);
// The one ordered sort of the exact path (dd_exact.hip): n keys radix-sorted by their 2k significant bits -- lo alone for
// k <= 32, (hi, lo) by two stable passes for k > 32 -- with `follow`, an array of follow_bytes (1 or 8) per key, taking the
// same permutation (null: keys only).  Every array has its other half of a double buffer; the result is in the _alt halves
// for k <= 32 (hi is not touched) and back in lo / hi / follow for k > 32.
size_t exact_sort_keys_temp_bytes(size_t n, int k, size_t follow_bytes);
hipError_t launch_exact_sort_keys(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, void* follow, void* follow_alt,
                                  size_t follow_bytes, size_t n, int k, void* temp, size_t temp_bytes, hipStream_t st);
size_t exact_sort_temp_bytes(size_t n, int k);
// counters[2] += number of distinct values among the n slots (unwritten slots hold all-ones)
hipError_t launch_exact_sort_count(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, size_t n,
                                   int k, void* temp, size_t temp_bytes, unsigned long long* counters,
                                   hipStream_t st);

// ---------------------------------------------------------------------------------------
// exact union schedules (dd_exact_sched.hip): extract with the genome's index -> radix sort -> per distinct k-mer a
// 64-bit membership mask -> the schedule's accumulator.  Counts are u64 and add up over passes and bins.
// ---------------------------------------------------------------------------------------
// how a k-mer carries its genome: 1 = top byte of its most significant word (2k, or 2k - 64, bits leave 8 free), 2 = a
// byte array next to the keys (k = 29..32, 61..64)
inline constexpr int exact_tag_mode(int k) { return (k <= 32 ? 2 * k : 2 * k - 64) <= 56 ? 1 : 2; }
constexpr int kExactSubsetsLdsN = 15;   // subsets: 2^n histogram bins in LDS (u32, 128 KiB at 15); n = 16 as two halves by the top bit
enum { kSchedPairwise = 0, kSchedProgressive = 1, kSchedLeaveOut = 2, kSchedSubsets = 3,
       kSchedSpectrum = 4, kSchedCoreProgressive = 5, kSchedSelect = 6,    // 4..6: the intersection schedules
       kSchedStream = 7,     // the masks themselves, kept in HBM for a walk that needs every k's masks at once (dd_exact_greedy.hip)
       kSchedPatterns = 8 }; // the distinct masks with their multiplicities, as (mask, count) pairs for dd_exact_patterns.hip
struct ExactSorted {            // where launch_exact_sort_tagged left the sorted k-mers
    const uint64_t* lo;
    const uint64_t* hi;         // k > 32
    const uint8_t* g;           // tag mode 2
};
struct ExactSched {
    int kind, n;
    int norder;                 // progressive, core-progressive: orderings; select: queries (any number >= 1);
                                // patterns: slots of a workgroup's LDS table, a power of two in kPatternSlotsMin..kPatternSlotsMax
    int ngroups;                // leave-out
    const uint64_t* table;      // device; progressive: prefix masks [norder][n]; leave-out: group of bit i [64] (~0: never left out),
                                //         then the groups' masks [ngroups]; core-progressive: the prefix masks of progressive;
                                //         select: (all, none) [norder][2]
    unsigned long long* acc;    // device, exact_sched_acc_words() of them, zeroed by the caller: [0] = M, the number of distinct k-mers,
                                //   pairwise: then |A_i n A_j| for i <= j, row by row (the diagonal: |A_i|)
                                //   progressive: then [norder][n] k-mers whose first genome of ordering o stands at position j
                                //   leave-out: then [ngroups] k-mers no genome outside group g holds
                                //   subsets: then [2^n] k-mers per membership mask
                                //   spectrum: then [n+1] k-mers held by exactly j genomes
                                //   core-progressive: then [norder][n] k-mers that hold genomes 0..j of ordering o and not genome j+1
                                //   select: then [norder] k-mers whose mask contains all[q] and meets none[q] nowhere
                                //   stream, patterns: nothing more
    // stream: every mask is appended to store[] at a position reserved on *cursor (one reservation per tile of masks, so their
    // order is whatever the reservations give); a tile that would pass `cap` sets *overflow and is not written, the cursor
    // still advances: it says how many masks the store would have had to hold
    uint64_t* store = nullptr;
    unsigned long long* cursor = nullptr;
    unsigned long long* overflow = nullptr;
    unsigned long long cap = 0;
    // patterns: (mask, count) pairs go to store[] / counts[] at positions reserved on *cursor, one reservation per flush of a
    // workgroup's table; the same capacity rule.  A pair stands for at least one distinct k-mer of the pass, so cap = the
    // slots of the pass is never passed.  pstats[0] += flushes a full table forced, pstats[1] += masks that left singly.
    unsigned long long* counts = nullptr;
    unsigned long long* pstats = nullptr;
};
size_t exact_sched_acc_words(const ExactSched& s);
size_t exact_sched_temp_bytes(size_t n, int k);
size_t exact_sched_scratch_bytes(size_t count);
hipError_t launch_exact_sort_tagged(uint64_t* lo, uint64_t* hi, uint64_t* lo_alt, uint64_t* hi_alt, uint8_t* g, uint8_t* g_alt,
                                    size_t n, int k, void* temp, size_t temp_bytes, hipStream_t st, ExactSorted* out);
hipError_t launch_exact_sched(const ExactSorted& sorted, size_t count, int k, const ExactSched& s, void* scratch, hipStream_t st);
// The union schedules for up to 255 genomes (dd_exact_wide.hip), behind launch_exact_sort_tagged like launch_exact_sched and
// with its contract: a row of W = exact_wide_words(n) <= 4 words per distinct k-mer where the narrow form has one mask.
struct ExactWide {
    int kind, n;                // kSchedPairwise, kSchedProgressive or kSchedLeaveOut; 1 <= n <= 255
    int norder;                 // progressive: orderings
    int ngroups;                // leave-out, <= 255
    const uint64_t* table;      // device; progressive: prefix rows [norder][n][W]; leave-out: group of bit i [256] (~0: never left
                                //         out), then the groups' rows [ngroups][W]
    unsigned long long* acc;    // device, exact_wide_acc_words() of them, zeroed by the caller: [0] = M, then what ExactSched's has
};
int exact_wide_words(int n);
size_t exact_wide_acc_words(const ExactWide& s);
size_t exact_wide_scratch_bytes(size_t count);   // (the temp of the sort is exact_sched_temp_bytes)
hipError_t launch_exact_wide(const ExactSorted& sorted, size_t count, int k, const ExactWide& s, void* scratch, hipStream_t st);
// The selected k-mers themselves (emit_kernel of dd_exact_sched.hip), behind launch_exact_sort_tagged and with the scratch
// of launch_exact_sched: every distinct k-mer whose mask matches at least one of the nq <= kEmitMaxQueries (all, none) pairs
// is appended once -- key in lo / hi (hi written for k > 32 only), mask in mask -- at a position reserved on *cursor, one
// reservation per chunk of the sorted array, so the order is whatever the reservations give.  A range that would pass `cap`
// records is not written; the cursor still advances and says how many records there were.
constexpr int kEmitMaxQueries = 1024;
struct ExactEmit {
    int n, nq;
    const uint64_t* table;       // device: (all, none) [nq][2]
    uint64_t *lo, *hi, *mask;    // device, [cap] each (null when cap = 0)
    unsigned long long* cursor;  // device, zeroed by the caller before the first pass; runs on across passes
    unsigned long long cap;
};
hipError_t launch_exact_emit(const ExactSorted& sorted, size_t count, int k, const ExactEmit& e, void* scratch, hipStream_t st);
// ... and put in ascending key order behind the last pass, for who wants an order (dd_exact_select_kmers) or searches them
// (dd_exact_locate).  `work`: exact_emit_order_bytes(found, k) of device memory; lo / hi / mask [found] are the emit area and
// are overwritten.
struct LocateSet {                  // where launch_exact_emit_order left the records, ascending in (hi, lo)
                                    // (named for its first user: locate_kernel takes it by value, a new name would change the kernel's symbol)
    const uint64_t* lo;
    const uint64_t* hi;             // k > 32
    const uint64_t* mask;
    unsigned long long found;
};
size_t exact_emit_order_bytes(size_t found, int k);
hipError_t launch_exact_emit_order(uint64_t* lo, uint64_t* hi, uint64_t* mask, size_t found, int k, void* work, hipStream_t st,
                                   LocateSet* out);

// ---------------------------------------------------------------------------------------
// the membership-pattern table (dd_exact_patterns.hip) behind kSchedPatterns: the pairs of a pass sorted by mask and reduced,
// the result merged into a running table in mask order, the table put in answer order behind the last pass.  rocPRIM on the
// caller's stream; every count is a u64.
// ---------------------------------------------------------------------------------------
constexpr int kPatternSlotsMin = 64, kPatternSlotsMax = 8192, kPatternSlotsDefault = 4096;   // 12 B of LDS per slot
struct PatternPairs {               // the pair area of a pass, carved from the scratch behind the sort's temp
    unsigned long long* head;       // [32]: cursor, overflow word, forced flushes, single masks; [4]: where a reduce leaves its row count
    uint64_t* mask;                 // [cap]
    unsigned long long* count;      // [cap]
    size_t cap;
    void* sched_scratch;            // exact_sched_scratch_bytes(keys) for launch_exact_sched
};
size_t exact_patterns_scratch_bytes(size_t keys);
size_t exact_patterns_temp_bytes(size_t keys, int k);   // the larger of the tagged sort's temp and the reduce's
PatternPairs exact_patterns_pairs(void* scratch, size_t keys);
// pairs [0, npairs) of `p`, masks of n bits -> rows in mask order, each mask once, back in p.mask / p.count; their number to p.head[4].
// alt_mask / alt_count: npairs words each (the k-mer arrays of the pass, which the schedule has consumed).
hipError_t launch_patterns_reduce(const PatternPairs& p, size_t npairs, int n, uint64_t* alt_mask, unsigned long long* alt_count, void* temp,
                                  size_t temp_bytes, hipStream_t st);
// table (rows_a, mask order) + rows of a pass (rows_b, mask order) -> a table in mask order at the front of `dst`
// (exact_patterns_merge_bytes(rows_a + rows_b) of device memory): masks at dst, counts at dst + patterns_stride(rows_a + rows_b);
// its row count to *rows_out (device, inside dst)
size_t exact_patterns_stride(size_t rows);
size_t exact_patterns_merge_bytes(size_t rows);
hipError_t launch_patterns_merge(const uint64_t* mask_a, const unsigned long long* count_a, size_t rows_a, const uint64_t* mask_b,
                                 const unsigned long long* count_b, size_t rows_b, void* dst, unsigned long long** rows_out, hipStream_t st);
// the table in answer order -- count descending, ties by mask ascending -- in `work` (exact_patterns_order_bytes(rows)):
// masks at work, INVERTED counts (~count) at work + exact_patterns_stride(rows)
size_t exact_patterns_order_bytes(size_t rows);
hipError_t launch_patterns_order(const uint64_t* mask, const unsigned long long* count, size_t rows, void* work, hipStream_t st);

// ---------------------------------------------------------------------------------------
// the positions of the selected k-mers (dd_exact_locate.hip), behind launch_exact_emit_order: every token of a painted
// genome looked up in the ordered records.
// ---------------------------------------------------------------------------------------
constexpr int kLocateJobs = 8;      // jobs one walk of a genome serves (a hit word each, in registers); more jobs: more units
struct LocateUnit {                 // one per gridDim.y of a launch, device-resident table
    const uint32_t* codes;          // the genome's token stream (ExactGenome)
    const uint32_t* bad;
    const unsigned long long* ntok;
    int nj, pad;                    // jobs of this unit, 1..kLocateJobs
    uint64_t all[kLocateJobs], none[kLocateJobs];
    unsigned long long out[kLocateJobs];   // first word of each job's bitmap in the hit buffer; ceil(ntok / 64) words follow
};
// every live thread writes its word of every job: the bitmaps need no zeroing.  Nothing is launched for an empty set.
void launch_exact_locate(const LocateUnit* units_dev, int nunits, size_t max_segments, int k, int canonical, const LocateSet& set,
                         uint64_t* hits_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, screened against the ordered records (dd_exact_screen.hip), behind launch_exact_emit_order.
// ---------------------------------------------------------------------------------------
constexpr int kScreenMaxQueries = 1024;   // (all, none) pairs one tally holds in LDS
// samples_dev[ns]: the samples' token streams (`base` is not read).  seen_dev [ns][words] u32, words >= ceil(found / 32),
// zeroed by the caller: bit r of row s is set iff sample s holds record r.  Nothing is launched for an empty set.
void launch_exact_screen(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set,
                         uint32_t* seen_dev, size_t words, hipStream_t st);
// shared_dev [ns + 1][n] += records of the row that hold bit i; match_dev [ns + 1][nq] += records of the row whose mask has
// (m & all) == all && (m & none) == 0 for pair q of table_dev [nq][2].  Row s < ns: the records seen by sample s; row ns:
// every record.  Both zeroed by the caller.
void launch_exact_tally(const LocateSet& set, const uint32_t* seen_dev, size_t words, int ns, int n, int nq, const uint64_t* table_dev,
                        unsigned long long* shared_dev, unsigned long long* match_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, painted window by window (dd_exact_paint.hip), behind launch_exact_emit_order.
// ---------------------------------------------------------------------------------------
constexpr int kPaintPlanes = 7;           // bit planes of a thread's per-genome counters: a segment ends at most 64 = 1000000b k-mers
constexpr size_t kPaintMaxWindow = (size_t)1 << 22;   // tokens of a window at the most (a multiple of kSegTokens, from kSegTokens on)
// samples_dev[ns]: the samples' token streams (`base` is not read).  counts_dev [rows][n + 2] u32, zeroed by the caller:
// sample s owns ceil(ntok_s / (64 window_segments)) rows from row0_dev[s] on, one per window of its token stream; row w,
// column 0 += the tokens of the window at which a valid k-mer ends, column 1 += those whose k-mer is a record of `set`,
// column 2 + i += those whose record's mask has bit i.  An empty set (found = 0, no array read) gives column 0 alone.
void launch_exact_paint(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set, int n,
                        size_t window_segments, const unsigned long long* row0_dev, uint32_t* counts_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, called row by row (dd_exact_reads.hip), behind launch_exact_emit_order: paint's walk and
// counters with rows from the caller's borders, then the vote over each row and the tally of the votes.
// ---------------------------------------------------------------------------------------
constexpr int kReadsClasses = 64 + 3;     // bins of a sample's tally: unique to genome i < n | ambiguous | unclassified | no valid k-mer
// samples_dev[ns]: the samples' token streams (`base` is not read).  off_dev [ns + 1]: sample s owns the rows off[s] ..
// off[s+1]-1 of start_dev and counts_dev; start_dev: row r of a sample covers its tokens start[r] .. start[r+1]-1, its last
// row runs to ntok -- strictly ascending within a sample and <= ntok (the caller has checked both), the tokens in front of a
// sample's first border in no row.  counts_dev [rows][n + 2] u32, zeroed by the caller: launch_exact_paint's columns, a
// k-mer counting in the row that holds its end token.  An empty set (found = 0, no array read) gives column 0 alone.
void launch_exact_reads(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set, int n,
                        const unsigned long long* off_dev, const unsigned long long* start_dev, uint32_t* counts_dev, hipStream_t st);
// Behind launch_exact_reads on the same stream.  calls_dev [rows][6] u32 (valid, hit, best, best_count, second,
// second_count; 0xFFFFFFFF: no such genome) and sets_dev [rows][2] u64 (ties, full): either may be null and is then not
// written.  tally_dev [ns][n + 3] u64, zeroed by the caller: += the rows of sample s in each class, a row with a valid k-mer
// being classified where its best column reaches min_hits.  max_rows: the rows of the sample that owns most.
void launch_exact_vote(const uint32_t* counts_dev, const unsigned long long* off_dev, int ns, size_t max_rows, int n, uint32_t min_hits,
                       uint32_t* calls_dev, uint64_t* sets_dev, unsigned long long* tally_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, counted record by record (dd_exact_depth.hip), behind launch_exact_emit_order: screen's walk
// with a counter where screen keeps a bit, then the counters binned by depth per genome and per query.
// ---------------------------------------------------------------------------------------
constexpr int kDepthMaxBins = 256;        // bins of a row's histogram at the most (the last one clipped)
constexpr size_t kDepthTileBytes = 72 * 1024;   // LDS of a tally workgroup's rows: two workgroups to a CU's 160 KiB
// samples_dev[ns]: the samples' token streams (`base` is not read).  count_dev [ns][found] u32, zeroed by the caller:
// += the tokens of sample s at which a valid k-mer ends that is record r.  A sample must hold fewer than 2^32 tokens (the
// caller has checked its bytes).  Nothing is launched for an empty set.
void launch_exact_depth(const ExactGenome* samples_dev, int ns, size_t max_segments, int k, int canonical, const LocateSet& set,
                        uint32_t* count_dev, hipStream_t st);
// the rows (genomes and queries) whose histograms of `bins` bins one tally workgroup holds in LDS
int exact_depth_rows_tile(int bins);
// Behind launch_exact_depth on the same stream.  Row i < n: the records whose mask has bit i; row n + q: those that match
// pair q of table_dev [nq][2].  hist_dev [ns][n + nq][bins] u64 += the records of the row that sample s holds d times, for
// 1 <= d < bins - 1, and bins - 1 times or more in the last bin; bin 0 is NOT written (the size of the row less the other
// bins).  over_dev [ns][n + nq] u64 += c - (bins - 1) over the row's records with c >= bins - 1.  Both zeroed by the caller;
// 2 <= bins <= kDepthMaxBins.
void launch_exact_depth_tally(const LocateSet& set, const uint32_t* count_dev, int ns, int n, int nq, int bins, const uint64_t* table_dev,
                              unsigned long long* hist_dev, unsigned long long* over_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, laid along the genomes of the universe (dd_exact_cover.hip), behind launch_exact_emit_order
// and launch_exact_depth: the record of every position of a target genome, once; then per sample the counters of
// launch_exact_depth gathered through it into rows of six columns per window of the target.
// ---------------------------------------------------------------------------------------
constexpr int kCoverColumns = 6;          // valid | covered | depth | private | private_covered | private_depth
constexpr uint32_t kCoverMaxClip = 1023;  // a depth counts as min(c, clip): a window of kPaintMaxWindow positions stays inside 32 bits
constexpr uint32_t kCoverNone = 0xFFFFFFFFu;      // an index word: no valid k-mer ends at this token
constexpr uint32_t kCoverPrivate = 0x80000000u;   // ... or the record's index, and this bit: its mask is exactly 1 << genome
struct CoverUnit {                  // one per gridDim.y of both launches, device-resident table
    const uint32_t* codes;          // the target's token stream (ExactGenome)
    const uint32_t* bad;
    const unsigned long long* ntok;
    unsigned long long index;       // first word of the target in the index; ceil(ntok / 64) * 64 words follow
    unsigned long long row0;        // first row of the target in a sample's rows; ceil(ntok / (64 window_segments)) follow
    int genome, pad;                // the target's bit in the masks
};
// index_dev: every live thread writes the kSegTokens words of its segment, the index needs no zeroing.  found < 2^31 (the
// caller has checked).  Nothing is launched for an empty set.
void launch_exact_cover_index(const CoverUnit* units_dev, int nunits, size_t max_segments, int k, int canonical, const LocateSet& set,
                              uint32_t* index_dev, hipStream_t st);
// Behind launch_exact_cover_index and launch_exact_depth on the same stream.  count_dev [ns][found] u32: launch_exact_depth's.
// rows_dev [ns][nrows][kCoverColumns] u32, zeroed by the caller: row u.row0 + w of sample s takes the tokens of window w of
// target u at which a valid k-mer ends, record r, c = count[s][r]: column 0 += 1, 1 += (c >= 1), 2 += min(c, clip), and
// 3, 4, 5 the same over the tokens whose word has kCoverPrivate.  1 <= clip <= kCoverMaxClip.
void launch_exact_cover(const CoverUnit* units_dev, int nunits, size_t max_segments, const uint32_t* index_dev, const uint32_t* count_dev,
                        size_t found, int ns, size_t window_segments, uint32_t clip, size_t nrows, uint32_t* rows_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// samples that are no leaves, explained by the genomes of the universe one by one (dd_exact_gather.hip), behind
// launch_exact_emit_order and launch_exact_depth: the greedy set cover over the records a sample holds, a pass over the
// records and a pick per step, the walk's state on the device.
// ---------------------------------------------------------------------------------------
constexpr int kGatherDone = -1;           // GatherState::last1 of a walk that has stopped
constexpr int kGatherSums = 3;            // a sample's sums: the open pick's depth | the records it holds | the sum of their depths
constexpr int kGatherOpenDepth = 0, kGatherHeld = 1, kGatherHeldDepth = 2;
struct GatherState {                // one per sample of the round; all-zero bytes are a fresh walk
    uint64_t taken;                 // bit b: input b is picked and its records are out of the walk
    int32_t last1;                  // 0: nothing picked yet; b + 1: input b is the last pick, its depth is still open (bit b is
                                    // not in `taken` yet); kGatherDone
    int32_t pad;
};
// One pass over the records for every sample of the round whose walk goes on.  count_dev [ns][found] u32: launch_exact_depth's.
// A record of sample s is live when count > 0 and mask & taken == 0.  sums_dev[s][kGatherOpenDepth] += the counters of the
// live records with bit `last`; step_dev[s][b] += the other live records with bit b, for every b < n outside
// taken | 1 << last; where nothing is picked yet, sums_dev[s][kGatherHeld] += the records with count > 0 and
// sums_dev[s][kGatherHeldDepth] += their counters.  step_dev [ns][64] and sums_dev [ns][kGatherSums] u64, zeroed by the
// caller in front of the first pass.  Nothing is launched for an empty set.
void launch_exact_gather(const LocateSet& set, const uint32_t* count_dev, int ns, int n, const GatherState* state_dev,
                         unsigned long long* step_dev, unsigned long long* sums_dev, hipStream_t st);
// Step t of 0 .. steps behind pass t on the same stream (t == steps: the closing one, which picks nothing).  Per sample:
// depth_dev[s][t - 1] = the open pick's depth sum, cleared, and the pick folded into `taken`; then, for t < steps, the argmax
// b of step_dev[s][0..63], the lowest index on a tie: with step_dev[s][b] >= min_hits (>= 1) pick_dev[s][t] = b,
// unique_dev[s][t] = step_dev[s][b] and b is the open pick; otherwise pick_dev[s][t] = -1 and the walk has stopped, as it
// has behind t == steps.  t == 0: shared_dev[s][0..n-1] = step_dev[s].  step_dev[s] is zeroed.  pick_dev [ns][steps] i32,
// unique_dev and depth_dev [ns][steps] u64 zeroed by the caller, shared_dev [ns][n] u64.
void launch_exact_gather_pick(int ns, int n, int t, int steps, uint32_t min_hits, GatherState* state_dev, unsigned long long* step_dev,
                              unsigned long long* sums_dev, int32_t* pick_dev, unsigned long long* unique_dev, unsigned long long* depth_dev,
                              unsigned long long* shared_dev, hipStream_t st);

// ---------------------------------------------------------------------------------------
// exact greedy walk (dd_exact_greedy.hip) over the mask streams of kSchedStream: one launch per step of the walk reads
// every stream once.  gain[kk][b] += masks of stream kk (store[seg.off[kk] .. seg.off[kk + 1])) that meet `chosen` nowhere
// and hold bit b, for every b < 64 (a bit of `chosen` gains 0).  gain_dev [K][64], zeroed by the caller.
// ---------------------------------------------------------------------------------------
constexpr int kGreedyMaxK = 64;
struct GreedySegments {
    int K;
    unsigned long long off[kGreedyMaxK + 1];   // ascending; off[K] = masks in the store
};
void launch_exact_greedy_gains(const uint64_t* store, const GreedySegments& seg, int n, uint64_t chosen, unsigned long long* gain_dev,
                               hipStream_t st);

// ---------------------------------------------------------------------------------------
// gzip inflated on the device: BGZF blocks (dd_ginflate.hip: one wave per block, text straight into the FASTA buffer) and
// single-member files in pieces (dd_gunzip.hip around the same decoder)
// ---------------------------------------------------------------------------------------
struct InflateJob {
    const uint8_t* in;          // the block: a whole gzip member (header, deflate data, CRC-32, ISIZE)
    uint32_t in_len;
    uint32_t out_len;           // its ISIZE (<= 65536)
    uint8_t* out;               // where its text goes
};
// one single-member gzip file of a batch, inflated on the device in pieces (dd_gunzip.hip: launch_gunzip_members)
struct RawFile {
    const uint8_t* in;          // the whole file on the device, 256-byte aligned
    uint32_t in_len;            // ... up to the end of THIS member (a file of several members: one RawFile each, same `in`)
    uint64_t first_bit;         // where its deflate data starts (behind the member's gzip header), counted from `in`
    uint32_t guess_bits;        // the block-start finder looks at one range of this many bits per piece
    uint32_t nguess;            // ranges = entries of this file in starts / lens / offs
    uint32_t piece0;            // its first entry there
    uint32_t isize;             // bytes of text (the member's ISIZE)
    uint16_t* sym;              // [nguess][range_syms] symbols (a byte, or 0x8000 | position in the 32 KiB in front of the piece):
                                //   a piece that starts in range j and runs over r ranges owns r x range_syms of them
    uint32_t range_syms;
    uint16_t* arena;            // [isize]: the symbols of pieces too long for their ranges (counted first, then written here)
    uint8_t* windows;           // what stands in the 32 KiB in front of every piece, in two levels (dd_gunzip.hip: piece_maps_kernel):
                                //   u16 [nguess][32768] maps relative to the piece's group start, u16 [ngroups][32768] the groups' own maps,
                                //   u8 [ngroups][32768] the windows at the groups' starts
    uint32_t group0, ngroups;   // groups of kPieceGroup ranges; group0 = this file's first group in the batch
    uint8_t* text;              // [isize] where the text goes
};
// one device-inflated text of a batch and what kseq's record rules ask of it (dd_fastq.hip)
struct TextJob {
    uint8_t* text;
    uint32_t n;
    uint32_t fastq;             // classed by its first bytes: 1 = four-line FASTQ expected, 0 = FASTA (no line may start with '+')
    uint32_t block0;            // its first 4 KiB block among the batch's
    uint32_t* blk_count;        // [blocks]: newlines per block, then their exclusive scan (FASTQ only)
    uint32_t* nl;               // [nl_cap]: the positions of its newlines
    uint32_t nl_cap;
    uint32_t* nl_total;
};
// OR-ed into *errors_dev when a text is not what its first bytes said (not a decoder refusal).  OR-ed, not added: one thread per
// offending RECORD raises it, and 2304 records x 2^24 is 9 x 2^32 = 0 -- a text with exactly that many odd records once came out
// "accepted" (scripts/fuzz_fastq.py, seed 510 draw 206)
constexpr uint32_t kNotFourLine = 0x1000000u;
void launch_text_rules(const TextJob* jobs_dev, int njobs, uint32_t nblocks, bool any_fastq, uint32_t* errors_dev, hipStream_t st);
size_t inflate_lds_bytes();
// starts_dev: npieces u64 (bit positions); tables_dev: four arrays of npieces u32 (lens, offs, over, abase), `stride` words apart
constexpr uint32_t kPieceGroup = 32;
constexpr uint32_t kSizeMismatch = 0x10000u;   // OR-ed into *errors_dev when a file's pieces do not add up to its ISIZE (decoder refusals ADD 1 each)
inline size_t gunzip_window_bytes(size_t nguess) {   // the `windows` area of a file with that many ranges
    const size_t ngroups = (nguess + kPieceGroup - 1) / kPieceGroup;
    return nguess * 65536 + ngroups * (65536 + 32768);
}
void launch_gunzip_members(const RawFile* files_dev, int nfiles, int npieces, int ngroups, int nchunks, uint64_t* starts_dev, uint32_t* tables_dev, size_t stride,
                           const uint32_t* chunk0_dev, uint32_t* crcs_dev, uint32_t* errors_dev, hipStream_t st);
// *errors_dev += blocks that did not decode (the caller falls back to the host decoder)
void launch_inflate_bgzf(const InflateJob* jobs_dev, int njobs, uint32_t* errors_dev, hipStream_t st);
// the decoder over the pieces of single-member files, for launch_gunzip_members (dd_gunzip.hip).  mode 3: symbols into the pieces' own
// ranges, lens / over written; 1: only count the text of the pieces marked in `over`; 2: write those into the arena at abase_dev
void launch_inflate_pieces(int mode, const RawFile* files_dev, int nfiles, int npieces, const uint64_t* starts_dev, uint32_t* lens_dev, uint32_t* over_dev,
                           const uint32_t* abase_dev, uint32_t* errors_dev, hipStream_t st);

// synthetic FASTA
void launch_synth(uint64_t seed, int gi, uint64_t nbases, int nrec, uint8_t* out_dev, hipStream_t st);
size_t synth_size(uint64_t nbases, int nrec);
// "realistic" mode (dd_synth.hip): contig table on the host, bytes on the device
std::vector<uint64_t> synth_realistic_table(uint64_t seed, uint64_t nbases);
void launch_synth_realistic(uint64_t seed, int gi, const uint64_t* tab_dev, uint32_t ncontigs, uint64_t total, uint8_t* out_dev,
                            hipStream_t st);

}  // namespace dd
