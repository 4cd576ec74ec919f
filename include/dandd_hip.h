/*
 * dandd_hip.h -- C ABI of libdandd_hip.so: the MI355X (gfx950) delta-sketching engine
 * that replaces DandD's shell-outs to `dashing sketch|union|card` and GNU `parallel`.
 *
 * Boundary being replaced (reference = jessicabonnie/dandd, paths under /root/reference):
 *   the seven subprocess call sites lib/sketch_classes.py:190,198 (leaf sketch),
 *   :221,229 (union), :268,274 (card) and lib/huffman_dandd.py:233 (the
 *   `parallel -j 95% '<cmd {}>' ::: k...` k-batch).  The reference has no FFI; its
 *   "plugin API" is a CLI + filesystem + stdout contract.  Each
 *   entry point below names the command line(s) it stands in for.  INTEGRATION.md
 *   shows the ctypes stub a DandD maintainer would add to lib/sketch_classes.py.
 *
 * Conventions: every function returns 0 on success or a negative DD_E* code; the
 * message is available from dd_last_error() (thread-local).  The caller owns every
 * buffer.  `dd_ctx` is opaque, bound to one GPU, and not thread-safe (one context
 * per thread/device).  There is NO CPU fallback: dd_create fails loudly when no
 * gfx950 device is usable.  Pointers named *_dev are device (HBM) addresses on the
 * context's GPU; all others are host addresses.  No torch types cross this boundary.
 *
 * Register layout: one byte per HyperLogLog register, m = 2^log2m registers per
 * sketch, `[K][m]` row-major for a k-sweep kmin..kmax (K = kmax-kmin+1).
 */
#ifndef DANDD_HIP_H
#define DANDD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DD_ABI_VERSION 4

#define DD_OK 0
#define DD_EINVAL (-1)   /* bad argument */
#define DD_ENODEV (-2)   /* no usable gfx950 device / HIP runtime error at create */
#define DD_EHIP (-3)     /* HIP runtime error during a call */
#define DD_EIO (-4)      /* file could not be read */
#define DD_ENOMEM (-5)

typedef struct dd_ctx dd_ctx;

int dd_abi_version(void);
const char *dd_last_error(void);

/* Replaces the per-process configuration of `dashing sketch -S <log2m> [--no-canon]`
 * (lib/sketch_classes.py:358-365; canon_command :20-29).  log2m in 4..20, k in 1..64
 * (Dashing itself stops at k=32, lib/huffman_dandd.py:109; 33..64 is this engine's
 * documented extension).  Returns NULL on failure. */
dd_ctx *dd_create(int device, int log2m, int canonical);
void dd_destroy(dd_ctx *);
/* Run all of this context's work on the given hipStream_t (NULL = default stream). */
int dd_set_stream(dd_ctx *, void *hip_stream);
int dd_synchronize(dd_ctx *);

/* ---- leaf sketch over a whole k-sweep ------------------------------------------
 * Replaces   parallel -j 95% ' dashing sketch -k{} -S <R> --prefix <dir> <fasta> ' ::: kmin..kmax
 * (lib/huffman_dandd.py:214-218 + lib/sketch_classes.py:351-366): ONE pass over the
 * FASTA bytes instead of one process per k.  regs[K][m] is overwritten. */
int dd_sketch_buffer(dd_ctx *, const uint8_t *fasta, size_t nbytes, int kmin, int kmax,
                     uint8_t *regs);
/* path may be plain or gzip-compressed (DandD's inputs are .fa/.fasta/.fna[.gz],
 * lib/species_specifics.py:93).  Files under 4 MiB: one read, .gz inflated on the host with zlib;
 * larger ones take dd_sketch_files' pipeline (below) as a directory of one. */
int dd_sketch_fasta(dd_ctx *, const char *path, int kmin, int kmax, uint8_t *regs);
/* Ingestion pipeline for a whole directory of genomes: `nthreads` loader threads (0 = auto) read
 * and inflate into pinned host buffers ahead of the GPU (bounded pool); a copy stream moves batch b+1
 * to the device and batch b-1's registers back while batch b is sketched; consecutive small files
 * share one launch (~128 MB per batch).  regs[nfiles][K][m] on the host.  Replaces the reference's
 * sequential per-genome loop (lib/huffman_dandd.py:402-407), each iteration of which re-inflates the
 * file once per k.  gzip files -- BGZF (bgzip) and ordinary single-member files of 1 MiB .. 1 GiB --
 * are copied compressed and inflated on the device, their CRC-32 and ISIZE checked; a block the device refuses sends the call through the host decoder, which
 * reports what is wrong (DD_NO_GPU_INFLATE=1: host decoder from the start).  FASTQ is accepted (kseq's
 * record rules: oracle/POLICIES.md P10). */
int dd_sketch_files(dd_ctx *, const char *const *paths, int nfiles, int kmin, int kmax,
                    uint8_t *regs, int nthreads);
/* statistics of the last dd_sketch_files call: wall time, time the GPU-driving thread waited for the loader
 * threads, number of batched launches, FASTA bytes sent to the device */
int dd_last_ingest_stats(dd_ctx *, double *wall_ms, double *loader_wait_ms, int *batches, uint64_t *bytes);
/* The text dd_sketch_files works on, for verification: the same pipeline (loaders, H2D, the device decoders of BGZF and
 * single-member .gz files, the host decoder and kseq's FASTQ rewrite where those apply), but every file's bytes AS THE
 * TOKENIZER IS ABOUT TO READ THEM are copied back into out[i] (caps[i] bytes of room; lens[i] = the text's length, also
 * when the buffer was too small: DD_EINVAL then).  For a .gz FASTA file that is exactly what `zcat` prints -- the check
 * that stands in for  zcat <fasta.gz> | cmp - <what dashing's gzread saw>  (lib/species_specifics.py:93: inputs are .gz). */
int dd_inflate_files(dd_ctx *, const char *const *paths, int nfiles, uint8_t *const *out, const size_t *caps,
                     size_t *lens, int nthreads);
/* Batched, HBM-resident form: ngenomes FASTA byte buffers already on the device,
 * regs_dev[ngenomes][K][m] on the device.  Asynchronous on the context's stream. */
int dd_sketch_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes,
                     int ngenomes, int kmin, int kmax, uint8_t *regs_dev);

/* ---- union -----------------------------------------------------------------------
 * Replaces   dashing union -z -o <out> <in1> ... <inN>   (lib/sketch_classes.py:368-373):
 * out[i] = max_j in[j][i], len bytes (any multiple of m, e.g. a whole [K][m] slab). */
int dd_union(dd_ctx *, const uint8_t *const *in, int n, size_t len, uint8_t *out);
int dd_union_device(dd_ctx *, const uint8_t *const *in_dev, int n, size_t len, uint8_t *out_dev);

/* ---- cardinality -----------------------------------------------------------------
 * Replaces   dashing card --presketched <path...>   (lib/sketch_classes.py:306-321):
 * 64-bin register histogram + Ertl maximum-likelihood estimate, one double per sketch. */
int dd_card(dd_ctx *, const uint8_t *regs, double *est);
int dd_card_batch(dd_ctx *, const uint8_t *regs /*[njobs][m]*/, int njobs, double *est);
int dd_card_batch_device(dd_ctx *, const uint8_t *regs_dev, int njobs, double *est /*host*/);
/* histogram only (device kernel), hist[njobs][64] on the host */
int dd_hist_batch_device(dd_ctx *, const uint8_t *regs_dev, int njobs, uint32_t *hist);
/* Ertl MLE of one 64-bin histogram (host arithmetic, IEEE double, no device needed) */
double dd_ertl_mle(const uint32_t hist[64], int log2m);

/* ---- progressive unions ----------------------------------------------------------
 * Replaces the flat prefix unions of DeltaTree.sketch_ordering
 * (lib/huffman_dandd.py:644-663): for ordering o and prefix length j,
 * card[o][j-1][kk] = |union of leaf[ord[o][0..j-1]]| at k = kmin+kk, computed as a
 * running byte-max (max is associative, so it equals the flat union bit for bit) -- or, from
 * log2m 18 on and for n <= 32, as a running AND of threshold bit planes with a popcount per prefix
 * (dd_pscan.hip): the same integers.  Register bytes must be <= 63. */
int dd_progressive(dd_ctx *, const uint8_t *leaf /*[n][K][m]*/, int n, int K,
                   const int32_t *orderings /*[norder][n]*/, int norder,
                   double *card /*[norder][n][K]*/);
int dd_progressive_device(dd_ctx *, const uint8_t *leaf_dev, int n, int K,
                          const int32_t *orderings, int norder, double *card);

/* ---- all-pairs unions ------------------------------------------------------------
 * Replaces the 2-way unions of DeltaTree.pairwise_spiders (lib/huffman_dandd.py:666-695):
 * card[i][j][kk] for i<j is |leaf_i U leaf_j|; card[i][i][kk] is |leaf_i|; the lower
 * triangle mirrors the upper.  From log2m 12 on the histograms behind the estimates are counted as int8
 * Gram matrices on the matrix cores (dd_gram.hip; F_ij(v) = sum_r [a_ir <= v][a_jr <= v]): the same
 * integers as the byte-max + histogram kernel.  Register bytes must be <= 63. */
int dd_pairwise(dd_ctx *, const uint8_t *leaf /*[n][K][m]*/, int n, int K,
                double *card /*[n][n][K]*/);
int dd_pairwise_device(dd_ctx *, const uint8_t *leaf_dev, int n, int K, double *card);

/* ---- the rectangle: new sketches against a slab ------------------------------------
 * |a_s U b_j| at every k column: card[na][nb][K].  a: [na][K][m], b: [nb][K][m], this context's log2m.  What
 * dd_pairwise on the na + nb rows behind one another holds at [s][na + j], without the two squares on its diagonal,
 * without a copy of b, and with an na x nb table; the same integers behind the same estimator.  From log2m 12 on the
 * histograms are counted on the matrix cores (dd_gram.hip: blocks of 64 rows of a against blocks of 64 rows of b; a last
 * block of a with at most 32 rows in a half-height form); below, and with DD_CROSS_STREAM=1, by a streaming kernel.
 * The histograms are taken in rounds over a's 64-row blocks: DD_CROSS_HIST_MB (1024 when unset; read on every call) is
 * what a round's histograms may take, one block at the least.  The argument rules are dd_pairwise's; register bytes
 * must be <= 63.  dd_cross_host_device takes a from host memory and b where it lies in HBM: new samples against a
 * resident slab. */
int dd_cross(dd_ctx *, const uint8_t *a, int na, const uint8_t *b, int nb, int K, double *card);
int dd_cross_device(dd_ctx *, const uint8_t *a_dev, int na, const uint8_t *b_dev, int nb, int K, double *card /*host*/);
int dd_cross_host_device(dd_ctx *, const uint8_t *a, int na, const uint8_t *b_dev, int nb, int K, double *card);

/* ---- leave-out unions ------------------------------------------------------------
 * Replaces the (n-1)-way unions of DeltaTree.find_delta_delta (lib/huffman_dandd.py:559-566), one per
 * left-out set and climb step:
 * card[g][kk] = |union of every leaf whose group != g| at k = kmin+kk, for g < ngroups; card[ngroups][kk] = |union of all|.
 * group[i] == -1: the leaf is in every union and is never left out.  A group that holds every leaf is an error.
 * One read of the slab: per register the largest value, a group that holds it and the largest value outside that
 * group give every complement's histogram as integer corrections of the full union's (dd_leaveout.hip): the same
 * integers as a byte-max + histogram per complement.  ngroups <= n.  Register bytes must be <= 63. */
int dd_leave_out(dd_ctx *, const uint8_t *leaf /*[n][K][m]*/, int n, int K,
                 const int32_t *group /*[n]*/, int ngroups, double *card /*[ngroups+1][K]*/);
int dd_leave_out_device(dd_ctx *, const uint8_t *leaf_dev, int n, int K,
                        const int32_t *group, int ngroups, double *card);

/* ---- all-subset unions ---------------------------------------------------------------
 * For `dandd abba`: every prefix of every ordering of the n leaves is a subset, so the unions of all 2^n subsets give
 * exact expectations over all n! orderings.
 * card[s][kk] = |union of the leaves i with bit i of s set| at k = kmin+kk, for s < 2^n; card[0][kk] = 0.0.
 * One pass over the slab per column chunk: threshold bit planes AND-ed over a lattice of (high, low) leaf subsets
 * (dd_subsets.hip), the same integers as a byte-max + histogram per subset.  1 <= n <= 16 (else DD_EINVAL).
 * Register bytes must be <= 63. */
int dd_subsets(dd_ctx *, const uint8_t *leaf /*[n][K][m]*/, int n, int K,
               double *card /*[2^n][K]*/);
int dd_subsets_device(dd_ctx *, const uint8_t *leaf_dev, int n, int K, double *card);

/* ---- extend unions ------------------------------------------------------------------
 * The one union schedule whose first operand is NOT a leaf: a base sketch against every listed leaf.
 * card[r][kk] = |base U leaf[rows[r]]| at k column kk.  base == NULL: the empty sketch (card = |leaf[rows[r]]|).
 * rows == NULL: all n leaves in order (nrows = n).  Entries of rows in 0..n-1, repeats allowed.
 * One read of the listed rows: where a leaf's register exceeds base's, its histogram differs from base's by one
 * register moved between two bins (dd_extend.hip): the same integers as a byte-max + histogram per row.
 * Register bytes must be <= 63. */
int dd_extend(dd_ctx *, const uint8_t *base /*[K][m]*/, const uint8_t *leaf /*[n][K][m]*/, int n, int K,
              const int32_t *rows /*[nrows]*/, int nrows, double *card /*[nrows][K]*/);
int dd_extend_device(dd_ctx *, const uint8_t *base_dev, const uint8_t *leaf_dev, int n, int K,
                     const int32_t *rows, int nrows, double *card /*host*/);

/* ---- greedy orderings ---------------------------------------------------------------
 * For `dandd greedy`: the ordering that adds at each step the candidate that raises (DD_GREEDY_MAX) or lowers
 * (DD_GREEDY_MIN) delta the most -- the steepest and the flattest growth curve.
 * cand[ncand]: distinct leaf rows, in tie-break order.  order[j] = cand[j] for j < nfixed (a given start, may be 0);
 * then order[j] = the candidate c not yet chosen that maximises (minimises) delta(order[0..j-1] + c), for j < nsteps,
 * nfixed <= nsteps <= ncand, nsteps >= 1.  card[j][kk] = |union of leaf[order[0..j]]| at k = kmin + kk.
 * THE SELECTION RULE (the host layer's object path implements the same one):
 *   delta of a set over the window = the largest card[kk] / (kmin + kk) in IEEE double, ties between k going to the
 *   LARGER k (best <= c / k, walking k upwards from best = 0);
 *   ties between candidates (equal delta as doubles) go to the candidate that comes FIRST in cand.
 * One dd_extend step per position inside the call; the running union stays on the device.
 * 1 <= kmin, kmin + K - 1 <= 64.  Register bytes must be <= 63. */
#define DD_GREEDY_MAX 0
#define DD_GREEDY_MIN 1
int dd_greedy(dd_ctx *, const uint8_t *leaf /*[n][K][m]*/, int n, int K, int kmin, int mode,
              const int32_t *cand /*[ncand]*/, int ncand, int nfixed, int nsteps,
              int32_t *order /*[nsteps]*/, double *card /*[nsteps][K]*/);
int dd_greedy_device(dd_ctx *, const uint8_t *leaf_dev, int n, int K, int kmin, int mode,
                     const int32_t *cand, int ncand, int nfixed, int nsteps, int32_t *order, double *card);

/* ---- exact distinct k-mer count (the KMC stand-in) --------------------------------------
 * Replaces   kmc -ci1 -cs2 -k<K> [-b] -fm <fasta> <db> <tmp>   +   kmc_tools complex (set union)
 * +   kmc_tools info <db> | grep 'total k-mers'   (lib/sketch_classes.py:395,444-448,453-465):
 * number of distinct (canonical, per the context) k-mers over ALL n inputs together, k in 1..64.
 * Uses 16 (k<=32) or 32 (k>32) bytes of HBM per input byte up to a budget of 24 GiB (DD_EXACT_MB overrides);
 * larger inputs are counted in passes over disjoint parts of the k-mer space, so a union of any number of
 * genomes that fits HBM as FASTA bytes can be counted.  After a count of inputs that hold a token,
 * dd_last_sketch_stats' third value is the number of passes it took (1: everything at once). */
int dd_exact_count_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n,
                          int k, uint64_t *distinct);
int dd_exact_count(dd_ctx *, const char *const *paths, int n, int k, uint64_t *distinct);

/* ---- exact union schedules -------------------------------------------------------------
 * The exact counterparts of dd_pairwise / dd_progressive / dd_leave_out / dd_subsets, for trees built with
 * `--exact` (lib/sketch_classes.py:444-465: one kmc_tools union + info per union there): numbers of distinct
 * (canonical, per the context) k-mers of unions of the n inputs, for every k in kmin..kmax (K columns, k in 1..64).
 * Inputs are read, uploaded and packed once per call, and the k-mers of all n inputs are sorted ONCE per k: every
 * distinct k-mer gets a 64-bit membership mask (bit i: input i holds it) and every union's count is a sum over those
 * masks (dd_exact_sched.hip).  So 1 <= n <= 64 (subsets: <= 16), else DD_EINVAL.  Empty inputs and inputs without a
 * k-mer of length k contribute nothing.  The HBM budget and the passes are those of dd_exact_count (DD_EXACT_MB);
 * dd_last_sketch_stats' third value is the number of passes of the k that took the most.
 *   pairwise     card[i][j][kk] = |input_i U input_j|, card[i][i][kk] = |input_i|, lower triangle mirrored
 *   progressive  card[o][j][kk] = |union of inputs ord[o][0..j]|; every ordering a permutation of 0..n-1
 *   leave_out    card[g][kk] = |union of the inputs whose group != g|, card[ngroups][kk] = |union of all|;
 *                group[i] == -1: never left out; a group that holds every input is an error
 *   subsets      card[s][kk] = |union of the inputs i with bit i of s set|, card[0][kk] = 0
 * The *_device forms take FASTA bytes already on the device, as dd_exact_count_device does (16-byte aligned). */
int dd_exact_pairwise(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, uint64_t *card /*[n][n][K]*/);
int dd_exact_progressive(dd_ctx *, const char *const *paths, int n, int kmin, int kmax,
                         const int32_t *orderings /*[norder][n]*/, int norder, uint64_t *card /*[norder][n][K]*/);
int dd_exact_leave_out(dd_ctx *, const char *const *paths, int n, int kmin, int kmax,
                       const int32_t *group /*[n]*/, int ngroups, uint64_t *card /*[ngroups+1][K]*/);
int dd_exact_subsets(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, uint64_t *card /*[2^n][K]*/);
int dd_exact_pairwise_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                             uint64_t *card);
int dd_exact_progressive_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                                const int32_t *orderings, int norder, uint64_t *card);
int dd_exact_leave_out_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                              const int32_t *group, int ngroups, uint64_t *card);
int dd_exact_subsets_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                            uint64_t *card);
/* Host arithmetic, no device needed: hist[mask] = number of k-mers with that membership mask (2^n bins, 1 <= n <= 16) ->
 * card[s] = total - (k-mers whose mask avoids s), by a subset-sum transform of the histogram. */
int dd_exact_subsets_from_hist(const uint64_t *hist /*[2^n]*/, int n, uint64_t *card /*[2^n]*/);

/* ---- exact union schedules for 65 to 255 inputs ---------------------------------------------
 * dd_exact_pairwise / _progressive / _leave_out with the limit on n lifted to what the sort carries: the input travels
 * with its k-mer as one byte (0xFF: the slot nothing wrote), so 1 <= n <= 255, else DD_EINVAL ("n=%d outside 1..255").
 * The same ONE sort per k; every distinct k-mer gets a membership ROW of ceil(n / 64) <= 4 words where the entries above
 * keep one 64-bit mask (dd_exact_wide.hip).  Argument lists, output shapes, the other argument rules and their messages
 * (k in 1..64, orderings that are permutations, group ids in -1..ngroups-1, a group that holds every input), the budget
 * (DD_EXACT_MB), the passes and dd_last_sketch_stats' third value are those of the entries above, and for n <= 64 so are
 * the numbers, byte for byte.  The entries above stay: their limit and its message are part of ABI version 4.  (At n = 64
 * the wide entries measure 1.00 to 1.02 x the narrow ones on the same buffers: profiles/exact_wide.txt.) */
int dd_exact_wide_pairwise(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, uint64_t *card /*[n][n][K]*/);
int dd_exact_wide_progressive(dd_ctx *, const char *const *paths, int n, int kmin, int kmax,
                              const int32_t *orderings /*[norder][n]*/, int norder, uint64_t *card /*[norder][n][K]*/);
int dd_exact_wide_leave_out(dd_ctx *, const char *const *paths, int n, int kmin, int kmax,
                            const int32_t *group /*[n]*/, int ngroups, uint64_t *card /*[ngroups+1][K]*/);
int dd_exact_wide_pairwise_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                                  uint64_t *card);
int dd_exact_wide_progressive_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                                     const int32_t *orderings, int norder, uint64_t *card);
int dd_exact_wide_leave_out_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                                   const int32_t *group, int ngroups, uint64_t *card);

/* ---- exact intersection schedules: core genome, k-mer spectrum, marker k-mers ------------------------------
 * What the union schedules cannot give and HyperLogLog sketches cannot estimate (inclusion-exclusion over 2^n union
 * estimates amplifies their error): counts of the distinct k-mers whose membership mask CONTAINS a set of inputs, or has
 * a given number of bits.  Same sort, same masks, same argument rules (1 <= n <= 64, k in 1..64), budget and passes as
 * the union schedules above; an empty input, or one without a k-mer of length k, holds nothing, so every core that
 * includes it is 0.
 *   spectrum          spec[j][kk] = distinct k-mers held by exactly j of the n inputs; spec[0][kk] = 0; the rows add
 *                     up to dd_exact_count of all inputs, spec[n] is the core of all
 *   core_progressive  core[o][j][kk] = k-mers held by every one of inputs ord[o][0..j]; every ordering a permutation of
 *                     0..n-1 (the rules of dd_exact_progressive); core[o][0] = |input ord[o][0]|, core[o][n-1] = spec[n]
 *   select            count[q][kk] = k-mers held by every input of all[q] and by no input of none[q] (bit i: input i);
 *                     any nq >= 1; a bit >= n set in all[q] or none[q]: DD_EINVAL; all = none = 0 counts every distinct
 *                     k-mer; all & none != 0 is legal and counts 0.  A group G of a clade: core (G, 0), private
 *                     (0, full ^ G), signature (G, full ^ G). */
int dd_exact_spectrum(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, uint64_t *spec /*[n+1][K]*/);
int dd_exact_core_progressive(dd_ctx *, const char *const *paths, int n, int kmin, int kmax,
                              const int32_t *orderings /*[norder][n]*/, int norder, uint64_t *core /*[norder][n][K]*/);
int dd_exact_select(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, const uint64_t *all /*[nq]*/,
                    const uint64_t *none /*[nq]*/, int nq, uint64_t *count /*[nq][K]*/);
int dd_exact_spectrum_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                             uint64_t *spec);
int dd_exact_core_progressive_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin,
                                     int kmax, const int32_t *orderings, int norder, uint64_t *core);
int dd_exact_select_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                           const uint64_t *all, const uint64_t *none, int nq, uint64_t *count);

/* ---- the selected k-mers themselves ---------------------------------------------------------------------------
 * dd_exact_select says how many k-mers match a query; this writes them.  ONE k per call (a range would need ragged
 * outputs), the sort and the masks of the schedules above, and the bit rules of dd_exact_select: a bit >= n set in all[q]
 * or none[q] is DD_EINVAL, all & none != 0 is legal and matches nothing, all = none = 0 matches every distinct k-mer.
 * 1 <= n <= 64, 1 <= k <= 64, 1 <= nq <= 1024 (what one launch holds; more is DD_EINVAL: split the queries over calls).
 * `found` must not be null; kmers and masks may be null only when cap == 0, which makes the call a pure count.
 *   *found    the number of distinct k-mers whose mask matches AT LEAST ONE query (a k-mer that matches several is one)
 *   found <= cap:  records 0 .. found-1 hold those k-mers in ASCENDING order of the 2k-bit key -- kmers[i][1] (hi: bits
 *             64 and up, 0 for k <= 32), then kmers[i][0] (lo), unsigned: two bits per base, A = 0, C = 1, G = 2, T = 3, the
 *             first base most significant, so the order is alphabetical -- and masks[i] is the membership mask of record i
 *             (bit j: input j holds it).  Two calls on the same inputs return identical bytes.
 *   found > cap:   the call still returns DD_OK; the contents of kmers and masks are then UNSPECIFIED (not a prefix of
 *             the answer), and the caller comes back with cap >= found.
 * The records wait in 24 bytes x min(cap, k-mer slots of the inputs) of HBM beside the exact workspace and are put in
 * order there, in the workspace itself (DD_ENOMEM with a message when either cannot be had); budget and passes are
 * those of dd_exact_count (DD_EXACT_MB), the count runs on across passes, dd_last_sketch_stats' third value is the
 * number of passes, and kernel time is DD_KERNEL_EXACT's.  An empty input, or one without a k-mer of length k, holds
 * nothing. */
int dd_exact_select_kmers(dd_ctx *, const char *const *paths, int n, int k, const uint64_t *all /*[nq]*/,
                          const uint64_t *none /*[nq]*/, int nq, uint64_t *kmers /*[cap][2]: lo, hi*/,
                          uint64_t *masks /*[cap]*/, size_t cap, uint64_t *found);
int dd_exact_select_kmers_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int k,
                                 const uint64_t *all, const uint64_t *none, int nq, uint64_t *kmers, uint64_t *masks,
                                 size_t cap, uint64_t *found);

/* ---- where the selected k-mers lie -----------------------------------------------------------------------------
 * dd_exact_select_kmers writes the k-mers that match a query; this says WHERE they stand in an input, without the k-mers
 * leaving the device (dd_exact_locate.hip).  ONE k per call, over the n inputs of the universe and a list of JOBS: job j
 * paints query (all[j], none[j]) onto input genome[j].  The bit rules are dd_exact_select's: a bit >= n set in all[j] or
 * none[j] is DD_EINVAL, all & none != 0 is legal and paints nothing, all = none = 0 paints every position where a valid
 * k-mer ends.  1 <= n <= 64, 1 <= k <= 64, 1 <= njobs <= 1024 (more is DD_EINVAL: split the jobs over calls), genome[j] in
 * 0..n-1.
 *   hits      job j owns the words off[j] .. off[j+1]-1: a bitmap over the tokens of input genome[j] as K0 lays them out
 *             (dd_fasta_index below), word w, bit b = token 64 w + b.  The bit is set iff a valid k-mer (no BREAK among its k
 *             tokens; canonical per the context) ENDS at that token and its membership mask m has (m & all) == all and
 *             (m & none) == 0.  Bits at or beyond the input's ntok are 0.  off[j+1] - off[j] must be ceil(ntok / 64) of
 *             input genome[j], else DD_EINVAL with a message naming the job and the number expected; hits may be null only
 *             when no word is asked for.  Nothing is written to hits unless the call returns DD_OK.
 *   *found    the number of distinct k-mers whose mask matches at least one job's query (dd_exact_select_kmers' meaning)
 * Two calls on the same inputs return identical bytes.  An input that is empty or shorter than k gets an all-zero bitmap.
 * The sort, the masks and the emission are dd_exact_select_kmers' (the jobs' distinct (all, none) pairs are its queries), so
 * are budget and passes (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer.  The records wait in
 * 24 bytes x the k-mer slots of the inputs of HBM (DD_ENOMEM with a message naming the bytes when that cannot be had) and
 * are put in key order there once, after the last pass, with the exact workspace as the sort's other half. */
int dd_exact_locate(dd_ctx *, const char *const *paths, int n, int k, const uint64_t *all /*[njobs]*/,
                    const uint64_t *none /*[njobs]*/, const int32_t *genome /*[njobs]*/, int njobs,
                    const uint64_t *off /*[njobs+1], in 64-bit words*/, uint64_t *hits /*[off[njobs]]*/, uint64_t *found);
int dd_exact_locate_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int k,
                           const uint64_t *all, const uint64_t *none, const int32_t *genome, int njobs,
                           const uint64_t *off, uint64_t *hits, uint64_t *found);
/* ---- samples screened against the universe ----------------------------------------------------------------------
 * Exact containment of files that are NOT inputs of the universe (dd_exact_screen.hip): which of the universe's k-mers a
 * sample holds, counted per input and per query, without the sample becoming a 65th mask bit, without its k-mers entering
 * the sort and without the universe's own numbers changing.  ONE k per call, 1 <= k <= 64, 1 <= n <= 64 universe inputs,
 * 1 <= ns <= 1024 samples, 0 <= nq <= 1024 queries (nq == 0: all, none and match may be null).  The bit rules are
 * dd_exact_select's: a bit >= n set in all[q] or none[q] is DD_EINVAL, all & none != 0 is legal and matches nothing,
 * all = none = 0 matches every record.  Counts are over DISTINCT k-mers (canonical per the context): a read set at 30x
 * coverage counts each k-mer once.
 *   shared[s][i]  s < ns: the distinct k-mers of sample s that universe input i also holds
 *   match[s][q]   s < ns: the distinct k-mers of sample s whose universe mask m has (m & all[q]) == all[q] and
 *                 (m & none[q]) == 0; with (0, 0): the k-mers of sample s that the universe holds at all
 *   row ns        of both arrays is the universe itself: shared[ns][i] = the distinct k-mers of input i, match[ns][q] what
 *                 dd_exact_select counts
 *   *found        the distinct k-mers of the universe
 * A sample that is empty, shorter than k or without a valid k-mer gives a zero row; a sample may be byte-identical to an
 * input.  The sample's own distinct count is not part of this entry (dd_exact_count gives it).  Nothing is written unless
 * the call returns DD_OK; two calls on the same inputs return identical bytes.  The device form takes n + ns buffers: the
 * n universe inputs first, the ns samples behind them.
 * The sort, the masks, the emission (always the single query (0, 0)) and the ordering are dd_exact_locate's, so are budget
 * and passes (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer; the samples are tokenised
 * with the universe but stay out of the sort and out of the slot count that sizes the record area.  Each sample's walk
 * marks the records it holds in a bitmap of ns x ceil(found / 32) x 4 bytes of HBM (DD_ENOMEM with a message naming the
 * bytes when that cannot be had); one tally of the marks gives every count. */
int dd_exact_screen(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                    const uint64_t *all /*[nq]*/, const uint64_t *none /*[nq]*/, int nq, uint64_t *shared /*[ns+1][n]*/,
                    uint64_t *match /*[ns+1][nq]*/, uint64_t *found);
int dd_exact_screen_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                           const uint64_t *all, const uint64_t *none, int nq, uint64_t *shared, uint64_t *match,
                           uint64_t *found);
/* ---- samples painted window by window ---------------------------------------------------------------------------
 * dd_exact_screen says how much of a sample each input holds; this says WHERE along the sample (dd_exact_paint.hip): the
 * token stream of every sample as K0 lays it out (dd_fasta_index below) is cut into windows of `window` tokens, window w
 * covering the tokens w * window .. (w + 1) * window - 1, and every window gets a row of n + 2 counters.  A k-mer belongs to
 * the window that holds its END token (dd_exact_locate's convention).  ONE k per call, 1 <= k <= 64, 1 <= n <= 64 universe
 * inputs, 1 <= ns <= 1024 samples; `window` a multiple of 64 in 64 .. 1 << 22, anything else is DD_EINVAL with a message.
 *   counts    sample s owns the rows off[s] .. off[s+1]-1, n + 2 columns of 32 bits each, counting the tokens of the window
 *             at which
 *               column 0      a valid k-mer ends (no BREAK among its k tokens; canonical per the context)
 *               column 1      that k-mer is a k-mer of the universe
 *               column 2 + i  that k-mer's membership mask has bit i: input i holds it
 *             Counts are over POSITIONS, not distinct k-mers: a k-mer that stands three times in a window counts three
 *             times (dd_exact_screen is the distinct count).  off[s+1] - off[s] must be ceil(ntok / window) of sample s, else
 *             DD_EINVAL with a message naming the sample and the number expected; counts may be null only when no row is
 *             asked for.  Nothing is written to counts unless the call returns DD_OK.
 *   *found    the distinct k-mers of the universe
 * An empty sample has no rows, one shorter than k has all-zero rows, an empty universe gives column 0 only; a sample may be
 * byte-identical to an input.  Two calls on the same inputs return identical bytes (integer sums).  The device form takes
 * n + ns buffers: the n universe inputs first, the ns samples behind them.
 * The sort, the masks, the emission (the single query (0, 0)) and the ordering are dd_exact_screen's, so are budget and
 * passes (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer; the samples are tokenised with the
 * universe but stay out of the sort and out of the slot count that sizes the record area.  The rows wait in
 * off[ns] - off[0] rows x (n + 2) x 4 bytes of HBM (DD_ENOMEM with a message naming the bytes when that cannot be had). */
int dd_exact_paint(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                   uint64_t window, const uint64_t *off /*[ns+1], in windows*/,
                   uint32_t *counts /*[off[ns]][n+2]*/, uint64_t *found);
int dd_exact_paint_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                          uint64_t window, const uint64_t *off, uint32_t *counts, uint64_t *found);
/* ---- samples called row by row -------------------------------------------------------------------------------------
 * dd_exact_paint cuts a sample into fixed windows; a read set, or a draft assembly, comes in records.  Here the rows are the
 * caller's (dd_exact_reads.hip): sample s owns the rows off[s] .. off[s+1]-1 (it may own none), and row r covers the tokens
 * start[r] .. start[r+1]-1 of the sample's token stream as K0 lays it out, the sample's last row running to its ntok; the
 * tokens in front of a sample's first border belong to no row.  With start = tok_start of dd_fasta_index the rows are the
 * file's records -- reads, contigs --, but the borders need not be record starts: the intervals of an annotation, or two
 * mates as one row, work as well.  A k-mer belongs to the row that holds its END token (dd_exact_locate's convention; K0
 * puts a BREAK in front of every record, so with record borders it lies whole inside that record).  ONE k per call,
 * 1 <= k <= 64, 1 <= n <= 64 universe inputs, 1 <= ns <= 1024 samples, min_hits >= 1; off must ascend, and within a sample
 * start must ascend strictly and stay <= that sample's ntok (start[first] = 0 is legal): anything else is DD_EINVAL with a
 * message, for the borders one that names the sample and the row.
 *   counts[r]  dd_exact_paint's columns for row r: column 0 the tokens of the row at which a valid k-mer ends, column 1 those
 *              whose k-mer the universe holds, column 2 + i those whose k-mer input i holds.  Counts are over POSITIONS.
 *   calls[r]   valid, hit (columns 0 and 1), best, best_count, second, second_count.  best: the input with the largest
 *              column, a tie to the lower index, 0xFFFFFFFF when hit == 0; second: the largest NON-ZERO column among the
 *              inputs other than best, a tie to the lower index, 0xFFFFFFFF (and a count of 0) when there is none.
 *   sets[r]    ties, full.  ties: the inputs whose column equals best_count, 0 when best_count == 0; full: the inputs whose
 *              column equals hit -- they hold every one of the row's universe positions --, 0 when hit == 0.
 *   The class of a row: no valid k-mer (valid == 0) | unclassified (valid > 0, best_count < min_hits) | unique
 *   (best_count >= min_hits, one bit in ties) | ambiguous (best_count >= min_hits, more than one bit in ties).
 *   tally[s]   [0 .. n-1] the rows of sample s uniquely called to input i, [n] the ambiguous, [n+1] the unclassified, [n+2]
 *              those without a valid k-mer: it sums to off[s+1] - off[s].  Voted and tallied on the device.
 *   *found     the distinct k-mers of the universe
 * tally and found must not be null.  calls, sets and counts may each be null: a null array is neither kept nor copied back,
 * and the tally-only call moves ns x (n + 3) x 8 bytes.  Nothing is written unless the call returns DD_OK.  An empty universe
 * gives column 0 only: every row with a valid k-mer is unclassified.  Two calls on the same inputs return identical bytes
 * (integer sums).  The device form takes n + ns buffers: the n universe inputs first, the ns samples behind them.
 * The sort, the masks, the emission and the ordering are dd_exact_screen's, so are budget and passes (DD_EXACT_MB),
 * dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer.  The rows wait in HBM: rows x (n + 2) x 4 bytes of
 * counters, rows x 8 of borders, rows x 24 and rows x 16 for calls and sets where asked for (DD_ENOMEM with a message
 * naming the bytes when that cannot be had; the rows are not chunked). */
int dd_exact_reads(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                   const uint64_t *off /*[ns+1], in rows*/, const uint64_t *start /*[off[ns]], tokens*/,
                   uint32_t min_hits, uint32_t *calls /*[off[ns]][6] or null*/, uint64_t *sets /*[off[ns]][2] or null*/,
                   uint32_t *counts /*[off[ns]][n+2] or null*/, uint64_t *tally /*[ns][n+3]*/, uint64_t *found);
int dd_exact_reads_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                          const uint64_t *off, const uint64_t *start, uint32_t min_hits, uint32_t *calls, uint64_t *sets,
                          uint32_t *counts, uint64_t *tally, uint64_t *found);
/* ---- samples counted record by record ---------------------------------------------------------------------------
 * dd_exact_screen counts a k-mer of the universe as present or absent in a sample; this says HOW MANY TIMES the sample holds
 * it (dd_exact_depth.hip), as a histogram of depths per universe input and per query.  For sample s and distinct k-mer r of
 * the universe, c[s][r] is the number of tokens of the sample's stream at which a valid k-mer ends that is r (canonical per
 * the context): POSITIONS, as in dd_exact_paint.  ONE k per call, 1 <= k <= 64, 1 <= n <= 64 universe inputs,
 * 1 <= ns <= 1024 samples, 0 <= nq <= 1024 queries (nq == 0: all and none may be null), 2 <= bins <= 256; the bit rules
 * are dd_exact_select's.  Row i < n takes the k-mers whose mask has bit i, row n + q those whose mask m has
 * (m & all[q]) == all[q] and (m & none[q]) == 0.
 *   hist[s][row][d]       d < bins - 1: the k-mers of the row with c == d; d = 0 are the k-mers of the row that the sample
 *                         lacks, so every row of hist sums to the size of the row (dd_exact_screen's row ns)
 *   hist[s][row][bins-1]  the k-mers of the row with c >= bins - 1 (the clipped bin)
 *   total[s][row]         the sum of c over the row's k-mers, unclipped
 *   *found                the distinct k-mers of the universe
 * A universe that holds no k-mer gives zeros; a sample that is empty or without a valid k-mer has everything in bin 0; a
 * sample may be byte-identical to an input.  Nothing is written unless the call returns DD_OK; two calls on the same inputs
 * return identical bytes (integer sums).  The device form takes n + ns buffers: the n universe inputs first, the ns samples
 * behind them.  A depth is a 32-bit counter: a sample of 2^32 bytes or more is DD_EINVAL.
 * The sort, the masks, the emission, the ordering and the sizes of the rows are dd_exact_screen's and are paid once per
 * call, so are budget and passes (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer.  The
 * samples are taken in rounds: as many as DD_DEPTH_MB (read on every call, MiB, 8192 unless set) holds of found x 4 bytes
 * of counters and (n + nq) x (bins + 1) x 8 bytes of histograms each.  A budget that does not hold one sample, or memory
 * that cannot be had, is DD_ENOMEM with a message naming the bytes. */
int dd_exact_depth(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                   const uint64_t *all /*[nq]*/, const uint64_t *none /*[nq]*/, int nq, int bins,
                   uint64_t *hist /*[ns][n+nq][bins]*/, uint64_t *total /*[ns][n+nq]*/, uint64_t *found);
int dd_exact_depth_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                          const uint64_t *all, const uint64_t *none, int nq, int bins, uint64_t *hist, uint64_t *total,
                          uint64_t *found);
/* ---- samples laid along the genomes of the universe ----------------------------------------------------------------
 * dd_exact_paint says where along a SAMPLE the universe's k-mers lie, dd_exact_depth how many times a sample holds the
 * k-mers of an input as a whole; this says where along an INPUT the sample lies, and how deep (dd_exact_cover.hip): the
 * coverage track of a read-mapping workflow, exact and alignment-free.  target[t] names an input of the universe; its token
 * stream as K0 lays it out (dd_exact_paint's, dd_fasta_index gives the records' places) is cut into windows of `window`
 * tokens, and every window gets, per sample, a row of six counters.  A k-mer belongs to the window that holds its END token.
 * With c the depth dd_exact_depth counts -- the positions of the sample at which the k-mer stands -- the columns count the
 * tokens of the window
 *   column 0  valid            at which a valid k-mer of the target ends (the same for every sample)
 *   column 1  covered          ... with c >= 1
 *   column 2  depth            the sum of min(c, clip) over them
 *   column 3  private          whose k-mer's membership mask is exactly 1 << target[t]: no other input holds it (the same
 *                              for every sample)
 *   column 4  private_covered  ... of those, with c >= 1
 *   column 5  private_depth    the sum of min(c, clip) over those
 * The clip keeps one repeat from carrying a window's mean, and a window of 2^22 positions inside 32 bits; with clip == 1
 * columns 2 and 5 equal columns 1 and 4.  ONE k per call, 1 <= k <= 64, 1 <= n <= 64 universe inputs, 1 <= ns <= 1024
 * samples, 1 <= nt <= n targets in 0..n-1, each once (a repeat is DD_EINVAL naming both places); `window` a multiple of 64 in
 * 64 .. 1 << 22; 1 <= clip <= 1023; off must ascend and off[t+1] - off[t] be ceil(ntok / window) of input target[t], else
 * DD_EINVAL with a message naming the target and the number expected; a sample of 2^32 bytes or more is DD_EINVAL
 * (dd_exact_depth's counter).  Sample s owns counts[s][off[0] .. off[nt]-1] of off[nt] rows; counts may be null only when
 * no row is asked for.
 *   *found    the distinct k-mers of the universe
 * A target without a token owns no rows, one shorter than k has all-zero rows, a universe without a k-mer gives zeros, an
 * empty sample gives columns 0 and 3 only; a sample may be byte-identical to an input, which it then covers everywhere.
 * Nothing is written unless the call returns DD_OK; two calls on the same inputs return identical bytes (integer sums).
 * The device form takes n + ns buffers: the n universe inputs first, the ns samples behind them.
 * The sort, the masks, the emission, the ordering and the counters are dd_exact_depth's, so are budget and passes
 * (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer.  The record of every target position is
 * looked up once per call and kept in 4 bytes x the targets' token slots of HBM; the samples are then taken in rounds: as
 * many as DD_DEPTH_MB (dd_exact_depth's variable) holds of found x 4 bytes of counters and off[nt] x 24 bytes of rows each.
 * An index word holds a record below 2^31: a universe of 2^31 distinct k-mers or more is DD_EINVAL.  A budget that does not
 * hold one sample, or memory that cannot be had, is DD_ENOMEM with a message naming the bytes. */
int dd_exact_cover(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                   const int32_t *target /*[nt]*/, int nt, uint64_t window, uint32_t clip,
                   const uint64_t *off /*[nt+1], in windows*/, uint32_t *counts /*[ns][off[nt]][6]*/, uint64_t *found);
int dd_exact_cover_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                          const int32_t *target, int nt, uint64_t window, uint32_t clip,
                          const uint64_t *off, uint32_t *counts, uint64_t *found);
/* ---- samples explained by the inputs of the universe, one by one ------------------------------------------------------
 * Every call above counts each input against the whole sample, independently: a sample that holds g3 shows a large
 * containment in g3's close relative too.  This says how FEW inputs explain what a sample shares with the universe, and in
 * what proportions (dd_exact_gather.hip): the greedy minimum set cover over the sample's k-mers, exact, integers only.
 * For one sample: H is the set of distinct k-mers r of the universe that the sample holds, d_r = c[s][r] > 0 the depth
 * dd_exact_depth counts; bit b of mask_r is input b.  taken_0 = 0, and at step t = 0, 1, ... for every input b
 *     U_t[b] = #{ r in H : mask_r & taken_t == 0 and bit b of mask_r }
 * The pick is b* = argmax_b U_t[b], ties to the LOWEST b.  The walk stops when U_t[b*] < min_hits or t == steps; otherwise
 * taken_{t+1} = taken_t | 1 << b* and
 *   pick[s][t]    b*
 *   unique[s][t]  U_t[b*]: the k-mers of the sample that b* holds and no earlier pick does; it never increases along t
 *   depth[s][t]   the sum of d_r over exactly those k-mers
 * and behind the stop pick = -1, unique = 0, depth = 0.  By-products of the first step:
 *   shared[s][b]  U_0[b], dd_exact_screen's shared[s][b]
 *   total[s][0]   |H|;  total[s][1]  the sum of d_r over H  (with min_hits == 1 and steps == n the sums of unique[s] and of
 *                 depth[s] equal them)
 *   *found        the distinct k-mers of the universe
 * An input that duplicates an earlier pick is never picked.  ONE k per call, 1 <= k <= 64, 1 <= n <= 64 universe inputs,
 * 1 <= ns <= 1024 samples; then min_hits >= 1; then 1 <= steps <= n; then no output may be null; then, in the device form,
 * the buffers, and a sample of 2^32 bytes or more is DD_EINVAL (dd_exact_depth's counter).  A universe that holds no k-mer,
 * an empty sample and a sample that shares nothing give every pick = -1 and zeros.  Nothing is written unless the call
 * returns DD_OK; two calls on the same inputs return identical bytes (integer sums).  The device form takes n + ns buffers:
 * the n universe inputs first, the ns samples behind them.
 * The sort, the masks, the emission, the ordering and the counters are dd_exact_depth's, so are budget and passes
 * (DD_EXACT_MB), dd_last_sketch_stats' third value and the DD_KERNEL_EXACT timer.  The walk runs on the device, one pass
 * over the sample's counters and one pick per step, with no host round trip inside it; the samples are taken in rounds: as
 * many as DD_DEPTH_MB (dd_exact_depth's variable) holds of found x 4 bytes of counters and the few hundred bytes of a walk
 * each.  A budget that does not hold one sample, or memory that cannot be had, is DD_ENOMEM with a message naming the bytes. */
int dd_exact_gather(dd_ctx *, const char *const *paths, int n, const char *const *samples, int ns, int k,
                    uint32_t min_hits, int steps, int32_t *pick /*[ns][steps]*/, uint64_t *unique /*[ns][steps]*/,
                    uint64_t *depth /*[ns][steps]*/, uint64_t *shared /*[ns][n]*/, uint64_t *total /*[ns][2]*/,
                    uint64_t *found);
int dd_exact_gather_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int ns, int k,
                           uint32_t min_hits, int steps, int32_t *pick, uint64_t *unique, uint64_t *depth,
                           uint64_t *shared, uint64_t *total, uint64_t *found);
/* ---- the membership-pattern table ------------------------------------------------------------------------------
 * Which sets of inputs share k-mers, and how many: the DISTINCT membership masks of the universe with their multiplicities
 * (the table behind an UpSet plot; every other mask statistic above -- spectrum, select, a subset union -- is a sum over
 * it).  ONE k per call (the outputs are ragged), 1 <= n <= 64, 1 <= k <= 64; the sort and the masks of the schedules above,
 * a hash table per workgroup in LDS as the accumulator (dd_exact_sched.hip), and the (mask, count) pairs it leaves sorted,
 * reduced and merged on the device (dd_exact_patterns.hip).  `found` must not be null; masks and counts may be null only when
 * cap == 0, which makes the call a pure count.
 *   *found    the number of distinct non-zero masks
 *   rows 0 .. min(found, cap) - 1:  masks[i] (bit j: input j holds the k-mers of this row) and counts[i], the distinct
 *             k-mers with exactly that mask, in the order COUNT DESCENDING, ties by MASK ASCENDING (unsigned).
 *   found > cap:  UNLIKE dd_exact_select_kmers the call returns DD_OK WITH A VALID PREFIX: the whole table is on the device
 *             anyway, and the cap rows written are the first cap rows of the full answer (the top-cap patterns).
 *   stats     null, or 4 words: [0] the distinct k-mers seen (the sum of every count of the table), [1] the pairs the
 *             workgroups wrote to HBM, [2] the flushes a full LDS table forced, [3] the masks written through singly.
 * Two calls on the same inputs return identical bytes.  An empty input, or one without a k-mer of length k, sets no bit;
 * when no input holds a k-mer, *found = 0.  Budget and passes are those of dd_exact_count (DD_EXACT_MB): the pairs of a
 * pass wait in 16 bytes per k-mer slot of the pass inside the exact workspace -- a pass writes at most one pair per distinct
 * k-mer, so that never overflows -- and the running table is kept beside the workspace, 16 bytes per row (DD_ENOMEM with a
 * message naming the bytes when it cannot be had).  dd_last_sketch_stats' third value is the number of passes, kernel time
 * is DD_KERNEL_EXACT's.  DD_PATTERNS_SLOTS (read on every call): the slots of a workgroup's table, a power of two in
 * 64..8192, 4096 when unset; anything else is DD_EINVAL. */
int dd_exact_patterns(dd_ctx *, const char *const *paths, int n, int k, uint64_t *masks /*[cap]*/,
                      uint64_t *counts /*[cap]*/, size_t cap, uint64_t *found, uint64_t *stats /*[4] or null*/);
int dd_exact_patterns_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int k,
                             uint64_t *masks, uint64_t *counts, size_t cap, uint64_t *found, uint64_t *stats);
/* Host only, no context and no device: names, sequence lengths and token starts of the records of one FASTA / FASTQ file,
 * plain or gzip, read by the loaders and record rules the exact calls and dd_sketch_files use.  K0 puts one BREAK token
 * where each header line ends -- IN FRONT of its record's bases -- and one for every ambiguous byte, so
 *   tok_start[r]  the index in the file's token stream of the first base of record r (of where it would be: an empty
 *                 record's is the next record's BREAK, or ntok); tok_start[0] = 1
 *   seq_len[r]    its bases, ambiguous ones included
 *   *ntok         the length of the stream = records + bases
 *   names         the first words of the header lines, NUL-terminated, one after the other; *names_need their bytes
 * *nrec > cap or *names_need > names_cap is DD_OK and a count, as found > cap is for dd_exact_select_kmers: the array that
 * lacks room is not written and the caller comes back with room. */
int dd_fasta_index(const char *path, uint64_t *seq_len /*[cap]*/, uint64_t *tok_start /*[cap]*/, size_t cap, uint64_t *nrec,
                   char *names, size_t names_cap, size_t *names_need, uint64_t *ntok);

/* ---- exact greedy orderings -----------------------------------------------------------------------------------
 * dd_greedy on exact counts, for `dandd greedy` on trees built with `--exact`: the same walk, the same SELECTION RULE
 * (above, word for word: the largest card[kk] / (kmin + kk) in IEEE double, ties between k to the LARGER k, ties between
 * candidates to the one that comes FIRST in cand), over numbers of distinct k-mers instead of estimates.
 * cand[ncand]: distinct inputs in 0..n-1, in tie-break order; order[j] = cand[j] for j < nfixed; nfixed <= nsteps <= ncand,
 * nsteps >= 1; mode DD_GREEDY_MAX or DD_GREEDY_MIN.  card[j][kk] = |union of inputs order[0..j]| at k = kmin + kk, exact.
 * Inputs that are not in cand are never chosen and contribute nothing.  1 <= n <= 64 and k in 1..64, as for the schedules
 * above; an empty input, or one without a k-mer of length k, holds nothing at that k.
 * The k-mers are sorted ONCE per k, as for the schedules (same budget and passes: DD_EXACT_MB), and what the sort leaves --
 * one 64-bit membership mask per distinct k-mer -- is kept in HBM for every k of the window, because a step picks by the
 * largest card / k over the WHOLE window: with C the inputs chosen so far,
 *     |C U c|_k = |C|_k + #{ masks m of k : m & C == 0 and bit c of m }
 * so a step is one read of the stored masks (dd_exact_greedy.hip) and no further sort.  The store has a budget of its own,
 * 24 GiB (DD_EXACT_MASKS_MB overrides; 8 bytes per distinct k-mer and k).  When the masks of the window do not fit it the
 * call returns DD_ENOMEM -- the message gives the masks needed so far and the budget -- and writes nothing to order or card:
 * there is no partial result. */
int dd_exact_greedy(dd_ctx *, const char *const *paths, int n, int kmin, int kmax, int mode,
                    const int32_t *cand /*[ncand]*/, int ncand, int nfixed, int nsteps,
                    int32_t *order /*[nsteps]*/, uint64_t *card /*[nsteps][K]*/);
int dd_exact_greedy_device(dd_ctx *, const uint8_t *const *fasta_dev, const size_t *nbytes, int n, int kmin, int kmax,
                           int mode, const int32_t *cand, int ncand, int nfixed, int nsteps, int32_t *order,
                           uint64_t *card);

/* ---- measurement hooks (bench.py) -------------------------------------------------
 * When enabled, every launch of kernel `which` is bracketed by HIP events on the
 * context's stream.  dd_timing_read synchronises the stream and returns the summed
 * device time and the number of launches since the last reset. */
#define DD_KERNEL_PACK 0
#define DD_KERNEL_SWEEP 1
#define DD_KERNEL_UNION 2
#define DD_KERNEL_EXACT 3 /* extract + sort + count / reduce + accumulate of dd_exact_count* and the dd_exact_* schedules; the steps of dd_exact_greedy; the emission and ordering of dd_exact_select_kmers; the emission, ordering and lookup of dd_exact_locate; the same and the tally of dd_exact_screen; the emission, ordering and window walk of dd_exact_paint; the emission, ordering, row walk and vote of dd_exact_reads; the emission, ordering, counting walk and depth tally of dd_exact_depth (every round); the same walk, the index and the window gather of dd_exact_cover; the same walk and the passes and picks of dd_exact_gather; the accumulation, merges and ordering of dd_exact_patterns */
#define DD_KERNEL_COUNT 4 /* the number of timed kinds, not a kind */
int dd_timing_enable(dd_ctx *, int on);
int dd_timing_read(dd_ctx *, int which, double *total_ms, int *launches);
int dd_timing_reset(dd_ctx *);
/* per-call statistics of the last dd_sketch_* call: tokens (bases + breaks) packed,
 * register updates issued (tokens x K upper bound), number of sweep workgroups */
int dd_last_sketch_stats(dd_ctx *, uint64_t *tokens, uint64_t *updates, int *sweep_blocks);
/* which kernels the last dd_progressive* / dd_pairwise* call of the context ran (ABI 3): the union schedules of
 * lib/huffman_dandd.py:644-695 have two device forms each, picked by register count and set sizes -- a benchmark
 * line must name the one that ran, not the one its author expected */
#define DD_K2_NONE 0
#define DD_K2_PROGRESSIVE_STREAM 1 /* progressive_kernel: running byte-max, one LDS histogram per prefix  */
#define DD_K2_PROGRESSIVE_PSCAN 2  /* pscan_kernel: running AND of threshold bit planes (log2m >= 18, n <= 32) */
#define DD_K2_PAIRWISE_STREAM 3    /* pairwise_kernel: one LDS atomic per register per pair */
#define DD_K2_PAIRWISE_GRAM 4      /* gram_kernel: int8 Gram matrices on the matrix cores (log2m >= 12) */
#define DD_K2_CROSS_STREAM 5       /* cross_stream_kernel: one LDS atomic per register per (row of a, row of b) */
#define DD_K2_CROSS_GRAM 6         /* cross_kernel: the rectangle as int8 Gram blocks (log2m >= 12) */
int dd_last_k2_path(dd_ctx *);
/* how many gram_kernel / cross_kernel launches the last dd_pairwise* / dd_cross* call of the context enqueued, summed over
 * dd_cross's rounds; 0 when it took a streaming form.  The Gram forms cut their units into launches whose partial counts
 * fit DD_GRAM_PART_MB MiB (1024 when unset or <= 0; read on every call), one unit at the least. */
int dd_last_k2_launches(dd_ctx *);

/* ---- synthetic FASTA on the device (bench / tests) ----------
 * Byte-identical to oracle/dd_oracle.c:orc_synth_fasta for the same arguments. */
size_t dd_synth_size(uint64_t nbases, int nrec);
int dd_synth_fasta_device(dd_ctx *, uint64_t seed, int genome_index, uint64_t nbases, int nrec,
                          uint8_t *out_dev);
/* "realistic" mode: GC 35 %, 30 % soft-masked repeats (interspersed + tandem), 2 % N, contigs of 2..200 kbp; byte-identical
 * to oracle/dd_oracle.c:orc_synth_realistic_fasta.  The contig structure (and so the size) depends on the seed. */
size_t dd_synth_realistic_size(uint64_t seed, uint64_t nbases);
int dd_synth_realistic_device(dd_ctx *, uint64_t seed, int genome_index, uint64_t nbases, uint8_t *out_dev);

/* ---- the K1 job table of a sketch call, without running it (tests; needs no GPU) --------
 * What stands in for `parallel -j 95%`'s process-per-k scheduling (lib/huffman_dandd.py:214-218):
 * how dd_sketch_device would cut (genome x k x 65536-token tile) into workgroup jobs for genomes of
 * these sizes.  Writes at most `cap` jobs in launch order and returns how many there are (or a
 * negative DD_E* code).  kclass: -1 small-k bitmap class (k <= 9), -2 the exact k-mer sets of k = 10 (, 11)
 * at log2m >= 19 (one job per slice of the k-mer index space: `slice`), else the window class of the launch
 * (0: k <= 16, 1: <= 32, 3: 33..48, 2: 49..64); mode: 0 registers in LDS (log2m <= 16); 5 (log2m >= 17) registers in HBM
 * through scatter + chunk sort + replay, jobs listed epoch by epoch. */
typedef struct {
    int kclass, mode, lds_bytes;
    int genome, kfirst, nk;
    unsigned tile_begin, tile_end;
    int slice; /* big-bitmap class (kclass -2, log2m >= 19): the slice of k's index space the job records */
} dd_plan_job;
long dd_plan_sweep(int log2m, const size_t *nbytes, int ngenomes, int kmin, int kmax, dd_plan_job *out,
                   long cap);

/* ---- multi-GPU: one context = one process = one GPU; RCCL over xGMI -----------------------------------------
 * The reference's only parallelism is GNU parallel over k on one host (lib/huffman_dandd.py:217).  Here (genome x k)
 * sketch jobs are split over the GPUs of a node by the CALLER (every rank sketches its own genomes: no exchange), and
 * what crosses xGMI is
 *   dd_allreduce_max_u8   the root union: every rank's [K][m] slab of byte-max-merged registers, in place
 *                         (ncclAllReduce, ncclUint8, ncclMax) -- stands in for the N-way  dashing union -z -o <root> <all leaves>
 *                         (lib/sketch_classes.py:368-373) over leaves that live on different GPUs;
 *   dd_allgather_u8       every rank's leaf slabs, for the schedules that need all leaves on every rank
 *                         (dd_progressive*, dd_pairwise*): recv_dev[world][n].
 * Both run on the context's stream (dd_set_stream) and return once enqueued.  Rank 0 makes the 128-byte id with
 * dd_comm_unique_id and hands it to the other ranks by any means (a file, MPI, a socket); every rank then calls
 * dd_comm_init -- collectively -- on a context of the GPU it owns.  librccl.so is opened on first use (DD_RCCL_LIB names
 * another copy); a process that never calls these needs no RCCL. */
#define DD_COMM_ID_BYTES 128
int dd_comm_unique_id(uint8_t *id /* [DD_COMM_ID_BYTES] */);
int dd_comm_init(dd_ctx *, int rank, int world, const uint8_t *id);
int dd_comm_destroy(dd_ctx *);
/* world = 0: the context belongs to no communicator; the counters are the collectives issued since dd_comm_init */
int dd_comm_info(dd_ctx *, int *rank, int *world, unsigned long long *allreduces, unsigned long long *allgathers);
int dd_allreduce_max_u8(dd_ctx *, uint8_t *regs_dev, size_t n);
int dd_allgather_u8(dd_ctx *, const uint8_t *send_dev, size_t n, uint8_t *recv_dev /* [world][n] */);

#ifdef __cplusplus
}
#endif
#endif
